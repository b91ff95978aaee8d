// mfx_db_merge.cpp -- mfx_db_merge, mfx_db_merge_except: sorted, delta-coded databases combined window by window (include/merfin_amd.h; the
// windows: mfx_merge.h; the session: mfx_db_windows.h; the kernels: mfx_merge.hip).  decoded runs -> merged and combined ->
// stream_append_device; no table in between.
#include "mfx_db_windows.h"

#include <stdlib.h>
#include <string.h>

// every check of mfx_db_merge that needs no device: the arguments, the inputs (opened into `ins`), their k, the output's identity
static int merge_check(const char *const *in_paths, uint32_t n_in, const char *out_path, const mfx_db_merge_opts *o, MergeIns &ins) {
  if (!in_paths || !out_path || !o) return mfx_fail(MFX_E_INVAL, "mfx_db_merge: null argument");
  if (n_in == 0 || n_in > MFX_MERGE_MAX_INPUTS) return mfx_fail(MFX_E_INVAL, "mfx_db_merge: %u inputs (1 to %u)", n_in, MFX_MERGE_MAX_INPUTS);
  if (o->op != MFX_MERGE_SUM && o->op != MFX_MERGE_MAX && o->op != MFX_MERGE_MIN && o->op != MFX_MERGE_INTERSECT)
    return mfx_fail(MFX_E_INVAL, "mfx_db_merge: unknown operation %d (MFX_MERGE_SUM, _MAX, _MIN, _INTERSECT)", o->op);
  if (o->minV > o->maxV) return mfx_fail(MFX_E_INVAL, "mfx_db_merge: the filter keeps nothing (min %llu > max %llu)", (unsigned long long)o->minV, (unsigned long long)o->maxV);
  if (int rc = db_open_inputs(in_paths, n_in, "mfx_db_merge", nullptr, "the inputs are of one k", ins)) return rc;
  const int same = db_output_is_input(out_path, ins);
  if (same >= 0) return mfx_fail(MFX_E_INVAL, "mfx_db_merge: the output '%s' is the input '%s'", out_path, in_paths[same]);
  return MFX_OK;
}

// not_paths: the databases whose k-mers are not written (mfx_db_merge_except); they are opened behind the inputs, share their windows and are
// decoded with counts of 0, which the combine kernel takes as "this k-mer is barred".  n_not == 0: mfx_db_merge.
static int mfx_db_merge_impl(const char *const *in_paths, uint32_t n_in, const char *const *not_paths, uint32_t n_not, const char *out_path, const mfx_db_merge_opts *o,
                             mfx_db_merge_stats *st, uint64_t *n_subtracted) {
  const char *who = n_not ? "mfx_db_merge_except" : "mfx_db_merge";
  if (st) memset(st, 0, sizeof(*st));
  if (n_subtracted) *n_subtracted = 0;
  MergeIns ins;
  if (n_not && (!not_paths || (uint64_t)n_in + n_not > MFX_MERGE_MAX_INPUTS))
    return not_paths ? mfx_fail(MFX_E_INVAL, "mfx_db_merge_except: %u inputs and %u to subtract (%u files at the most)", n_in, n_not, MFX_MERGE_MAX_INPUTS)
                     : mfx_fail(MFX_E_INVAL, "mfx_db_merge_except: null argument");
  if (int rc = merge_check(in_paths, n_in, out_path, o, ins)) return rc;
  const int k = (int)ins[0]->h.k;
  uint64_t n_read = 0;
  for (uint32_t i = 0; i < n_in; ++i) n_read += ins[i]->h.n;
  for (uint32_t j = 0; j < n_not; ++j) {                         // (one at a time: a subtracted database that is the output is refused before the next is opened)
    if (int rc = db_open_inputs(not_paths + j, 1, who, nullptr, "the inputs and what is subtracted are of one k", ins)) return rc;
    if (db_output_is_input(out_path, ins, n_in + j) >= 0)
      return mfx_fail(MFX_E_INVAL, "mfx_db_merge_except: the output '%s' is the subtracted database '%s'", out_path, not_paths[j]);
  }
  // ---- the windows, and what the largest of them takes
  MergeWindows P;
  if (int rc = merge_plan_windows(ins, k, who, P)) return rc;
  mfx_db_writer *w = nullptr;
  if (int rc = db_open_streamed(out_path, k, &w)) return rc;
  WriterAbort guard{w};
  w->merging = true;
  if (P.max_pairs) {
    DeviceBack back;
    MFX_HIP(hipSetDevice(o->device));
    // own.p[0], p[1]: two buffers of cap pairs, the k-mers in front of the counts: decoded runs, merge levels, combined pairs behind the writer's
    // carry, and the packed words of the one that is free by then.  p[2]: the combine's tile offsets, then the stats.
    const uint64_t cap = P.max_pairs + MFX_DELTA_BLOCK, tiles = mfx_combine_tiles(P.max_pairs), small = (tiles + 1 + 3) * 8;
    MergeDecoder dec;
    DbDev own;
    uint64_t total = 0;
    if (hipError_t e = db_alloc(dec, P, n_in + n_not, own, {cap * 12, cap * 12, small}, &total))
      return mfx_fail(MFX_E_NOMEM, "%s: the buffers of a window of %lu pairs (%.3f GB) do not fit the device: %s; lower MFX_MERGE_RANGE", who, (unsigned long)P.max_pairs,
                      (double)total / 1e9, hipGetErrorString(e));
    uint64_t *bk[2] = {(uint64_t *)own.p[0], (uint64_t *)own.p[1]};
    uint32_t *bv[2] = {(uint32_t *)((char *)own.p[0] + cap * 8), (uint32_t *)((char *)own.p[1] + cap * 8)};
    uint64_t *d_tile = (uint64_t *)own.p[2], *d_stats = d_tile + tiles + 1;
    MFX_HIP(mfx_memset_now(d_stats, 0, 24));
    StreamDev S;
    if (int rc = stream_dev_init(S, w, cap, who, "MFX_MERGE_RANGE")) return rc;
    const bool timing = getenv("MFX_DB_TIMING") != nullptr;
    if (n_not) dec.zero_from = n_in;
    DbPass pass(ins.size());
    const int rc_pass = db_each_window(ins, P, k, who, dec, bk[0], bv[0], pass, [&](std::vector<MergeRun> &runs) -> int {
      double t0 = db_now(), t1;
      // ---- merge: one ascending run per input in buffer 0, then the pairwise tree
      int cur = 0;
      if (int rc = merge_tree(runs, bk, bv, cur)) return rc;
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
      if (n_out > M) return mfx_fail(MFX_E_HIP, "%s: the combined pairs of a window are damaged", who);
      if (n_out)
        if (int rc = stream_append_device(w, S, bk[cur ^ 1], bv[cur ^ 1], n_out, bk[cur], cap * 12, who, "MFX_MERGE_RANGE")) return rc;
      return MFX_OK;
    });
    w->t_read = pass.t_read; w->t_decode = pass.t_decode;
    if (st) st->windows = pass.windows;
    if (rc_pass) return rc_pass;
    uint64_t stats[3] = {0, 0, 0};
    MFX_HIP(hipMemcpy(stats, d_stats, 24, hipMemcpyDeviceToHost));
    if (st) { st->n_saturated = stats[0]; st->n_filtered = stats[1]; }
    if (n_subtracted) *n_subtracted = stats[2];
  }
  guard.w = nullptr;
  uint64_t n = 0;
  if (int rc = mfx_db_writer_close(w, &n)) return rc;
  if (st) { st->n_in = n_read; st->n_out = n; }
  return MFX_OK;
}

extern "C" int mfx_db_merge(const char *const *in_paths, uint32_t n_in, const char *out_path, const mfx_db_merge_opts *o, mfx_db_merge_stats *st) {
  return db_guard("mfx_db_merge", [&] { return mfx_db_merge_impl(in_paths, n_in, nullptr, 0, out_path, o, st, nullptr); });
}

extern "C" int mfx_db_merge_except(const char *const *in_paths, uint32_t n_in, const char *const *not_paths, uint32_t n_not, const char *out_path,
                                   const mfx_db_merge_opts *o, mfx_db_merge_stats *st, uint64_t *n_subtracted) {
  return db_guard("mfx_db_merge_except", [&] { return mfx_db_merge_impl(in_paths, n_in, not_paths, n_not, out_path, o, st, n_subtracted); });
}

extern "C" int mfx_db_merge_plan(const uint64_t *const *first, const uint64_t *n, uint32_t n_in, int k, uint64_t R, uint64_t *out, uint64_t cap, uint64_t *n_windows) {
  if (!first || !n || !n_windows || n_in == 0 || n_in > MFX_MERGE_MAX_INPUTS || k < 1 || k > MFX_MAX_K_NARROW) return mfx_fail(MFX_E_INVAL, "mfx_db_merge_plan: bad argument");
  return db_guard("mfx_db_merge_plan", [&] {
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
    return (int)MFX_OK;
  });
}
