// mfx_db_join.cpp -- the sorted-database calls that end in a reduction (include/merfin_amd.h; the session: mfx_db_windows.h).
// mfx_db_join_*: -completeness and -spectrum from two sorted databases, window by window: the decoded runs go to mfx_join_kernel
// (mfx_join.hip) and end in the piece sums or in the image, nothing is merged into memory or written.
// mfx_db_diploid: two haplotype assemblies against the reads (the rule: mfx_diploid.h; the kernels: mfx_diploid.hip): hap1's and hap2's runs
// are tagged, merged (mfx_merge_pairs_kernel) and compacted into the pair run; the read run stays where the decode left it and is joined
// against the pair run by mfx_join_kernel.
#include "mfx_db_windows.h"
#include "mfx_trio.h"
#include "mfx_diploid.h"
#include "mfx_pipe.h"

#include <stdlib.h>
#include <string.h>

namespace { enum JoinKind { JOIN_COMPLETENESS, JOIN_SPECTRUM }; }

static int db_join_impl(const char *read_path, const char *asm_path, const mfx_db_join_opts *o, JoinKind kind, double *total64, double *undrcpy64, uint64_t *img,
                        uint64_t *n_entries, mfx_db_join_stats *st) {
  const char *who = kind == JOIN_COMPLETENESS ? "mfx_db_join_completeness" : "mfx_db_join_spectrum";
  const double t_begin = db_now();
  if (st) memset(st, 0, sizeof(*st));
  // ---- every check that needs no device
  if (!read_path || !asm_path || !o || (kind == JOIN_COMPLETENESS ? (!total64 || !undrcpy64) : (!img || !n_entries))) return mfx_fail(MFX_E_INVAL, "%s: null argument", who);
  if (kind == JOIN_COMPLETENESS && o->n_prob && (!o->probK || !o->probP)) return mfx_fail(MFX_E_INVAL, "%s: null argument", who);
  if (kind == JOIN_SPECTRUM) {                                 // (mfx_spectrum_run's bounds and texts)
    if (o->copies < MFX_SPEC_MIN_COPIES || o->copies > MFX_SPEC_MAX_COPIES)
      return mfx_fail(MFX_E_INVAL, "%s: copies = %u is outside [%u, %u]", who, o->copies, MFX_SPEC_MIN_COPIES, MFX_SPEC_MAX_COPIES);
    if (o->max_mult < MFX_SPEC_MIN_MULT || o->max_mult > MFX_SPEC_MAX_MULT)
      return mfx_fail(MFX_E_INVAL, "%s: max_mult = %u is outside [%u, %u]", who, o->max_mult, MFX_SPEC_MIN_MULT, MFX_SPEC_MAX_MULT);
  }
  MergeIns ins;
  const char *paths[2] = {read_path, asm_path};
  if (int rc = db_open_inputs(paths, 2, "mfx_db_join", "the sorted join takes", "the inputs are of one k", ins)) return rc;
  const int k = (int)ins[0]->h.k;
  MergeWindows P;
  if (int rc = merge_plan_windows(ins, k, who, P)) return rc;
  const size_t cells = kind == JOIN_SPECTRUM ? (size_t)(o->copies + 2u) * (o->max_mult + 1u) : 0;
  // res: stats word [0] (the k-mers of both), then the 128 piece sums or the image and its entry counter
  const size_t res_words = 2 + (kind == JOIN_COMPLETENESS ? 128 : cells + 1);
  std::vector<uint64_t> res(res_words, 0);
  DbPass pass(2);
  double t_join = 0;
  if (P.max_pairs) {
    DeviceBack back;
    MFX_HIP(hipSetDevice(o->device));
    // own.p[0]: one buffer of cap pairs, the k-mers in front of the counts: the decoded runs.  p[1]: the result.  p[2], p[3]: the -prob table.
    const uint64_t cap = P.max_pairs + 1, np = o->n_prob && kind == JOIN_COMPLETENESS ? o->n_prob : 1;
    MergeDecoder dec;
    DbDev own;
    uint64_t total = 0;
    if (hipError_t e = db_alloc(dec, P, 2, own, {cap * 12, res_words * 8, np * sizeof(uint32_t), np * sizeof(double)}, &total))
      return mfx_fail(MFX_E_NOMEM, "%s: the buffers of a window of %lu pairs (%.3f GB) do not fit the device: %s; lower MFX_MERGE_RANGE", who, (unsigned long)P.max_pairs,
                      (double)total / 1e9, hipGetErrorString(e));
    uint64_t *d_keys = (uint64_t *)own.p[0], *d_res = (uint64_t *)own.p[1];
    uint32_t *d_vals = (uint32_t *)((char *)own.p[0] + cap * 8), *d_probK = (uint32_t *)own.p[2];
    double *d_probP = (double *)own.p[3];
    MFX_HIP(mfx_memset_now(d_res, 0, res_words * 8));
    if (kind == JOIN_COMPLETENESS && o->n_prob)
      if (int rc = db_upload_prob(o, d_probK, d_probP)) return rc;
    int grid = 1;                                                // the workgroups a CU holds at once (mfx_join.hip: LDS)
    if (int rc = db_grid(o->device, kind == JOIN_COMPLETENESS ? 4 : 2, &grid)) return rc;
    mfx_spectrum_args sa{};
    if (kind == JOIN_SPECTRUM) sa = db_spectrum_args(o->copies, o->max_mult, mfx_spec_lds_cols(o->copies, o->max_mult), d_res + 2);
    const bool timing = getenv("MFX_DB_TIMING") != nullptr;
    // the read run and the asm run of a window.  (One stream: the blocks of a window are copied behind the join of the window before it, whose
    // kernel runs while the host reads.)
    const int rc_pass = db_each_window(ins, P, k, who, dec, d_keys, d_vals, pass, [&](std::vector<MergeRun> &runs) -> int {
      const double t0 = db_now();
      const MergeRun a = runs[0], b = runs[1];
      if (kind == JOIN_COMPLETENESS)
        MFX_HIP(mfx_k_join_completeness(d_keys + a.off, d_vals + a.off, a.len, d_keys + b.off, d_vals + b.off, b.len, k, o->peak, o->n_prob, d_probK, d_probP,
                                        reinterpret_cast<double *>(d_res + 2), d_res, grid, nullptr));
      else
        MFX_HIP(mfx_k_join_spectrum(d_keys + a.off, d_vals + a.off, a.len, d_keys + b.off, d_vals + b.off, b.len, sa, o->minV, o->maxV, d_res, grid, nullptr));
      if (timing) MFX_HIP(hipStreamSynchronize(nullptr));
      t_join += db_now() - t0;
      return MFX_OK;
    });
    if (rc_pass) return rc_pass;
    MFX_HIP(hipMemcpy(res.data(), d_res, res_words * 8, hipMemcpyDeviceToHost));
  }
  // ---- what the windows held against what the files say, the image against its counter: no partial result is handed out
  if (int rc = pass.check(ins)) return rc;
  const std::vector<uint64_t> &got = pass.got;
  const uint64_t n_both = res[0];
  if (n_both > got[0] || n_both > got[1]) return mfx_fail(MFX_E_HIP, "%s: %lu k-mers in both inputs, more than an input holds", who, (unsigned long)n_both);
  if (kind == JOIN_SPECTRUM) {
    uint64_t sum = 0;
    for (size_t i = 0; i < cells; ++i) sum += res[2 + i];
    if (sum != res[2 + cells]) return mfx_fail(MFX_E_HIP, "%s: the image sums to %lu, the join counted %lu entries", who, (unsigned long)sum, (unsigned long)res[2 + cells]);
    const bool filtered = o->minV > 1 || o->maxV < 0xffffffffull;      // (a count is 1 at the least: no other filter makes a pair (0, 0))
    if (!filtered && sum != got[0] + got[1] - n_both)
      return mfx_fail(MFX_E_HIP, "%s: the join counted %lu entries, the inputs hold %lu distinct k-mers", who, (unsigned long)sum, (unsigned long)(got[0] + got[1] - n_both));
    memcpy(img, res.data() + 2, cells * 8);
    *n_entries = sum;
  } else {
    memcpy(total64, res.data() + 2, 64 * sizeof(double));
    memcpy(undrcpy64, res.data() + 2 + 64, 64 * sizeof(double));
  }
  if (st) {
    st->n_read = got[0]; st->n_asm = got[1]; st->n_both = n_both; st->windows = pass.windows;
    st->t_read = pass.t_read; st->t_decode = pass.t_decode; st->t_join = t_join; st->t_total = db_now() - t_begin;
  }
  return MFX_OK;
}

extern "C" int mfx_db_join_completeness(const char *read_path, const char *asm_path, const mfx_db_join_opts *o, double *total64, double *undrcpy64, mfx_db_join_stats *st) {
  return db_guard("mfx_db_join_completeness", [&] { return db_join_impl(read_path, asm_path, o, JOIN_COMPLETENESS, total64, undrcpy64, nullptr, nullptr, st); });
}

extern "C" int mfx_db_join_spectrum(const char *read_path, const char *asm_path, const mfx_db_join_opts *o, uint64_t *img, uint64_t *n_entries, mfx_db_join_stats *st) {
  return db_guard("mfx_db_join_spectrum", [&] { return db_join_impl(read_path, asm_path, o, JOIN_SPECTRUM, nullptr, nullptr, img, n_entries, st); });
}

extern "C" void mfx_db_join_grain(uint32_t *per_lane, uint32_t *tile) {
  if (per_lane) *per_lane = MFX_JOIN_PER;
  if (tile) *tile = MFX_JOIN_TILE;
}

extern "C" int mfx_db_join_host(const uint64_t *read_keys, const uint32_t *read_vals, uint64_t n_read, const uint64_t *asm_keys, const uint32_t *asm_vals, uint64_t n_asm,
                                uint64_t *keys, uint32_t *readV, uint32_t *asmV, uint64_t cap, uint64_t *n_pairs) {
  if ((n_read && (!read_keys || !read_vals)) || (n_asm && (!asm_keys || !asm_vals)) || !n_pairs || (cap && (!keys || !readV || !asmV)))
    return mfx_fail(MFX_E_INVAL, "mfx_db_join_host: null argument");
  return db_guard("mfx_db_join_host", [&] {
    uint64_t n = 0;
    mfx_join_host(read_keys, read_vals, n_read, asm_keys, asm_vals, n_asm, [&](bool have, uint64_t key, uint32_t rv, uint32_t av) {
      if (!have) return;
      if (n < cap) { keys[n] = key; readV[n] = rv; asmV[n] = av; }
      ++n;
    });
    *n_pairs = n;
    return (int)MFX_OK;
  });
}

// ---- mfx_db_diploid -------------------------------------------------------------------------------------------------------------
static void diploid_fill_stats(const uint64_t *c, mfx_db_diploid_stats *st) {
  mfx_diploid_counts *x[3] = {&st->hap1, &st->hap2, &st->both};
  for (int i = 0; i < 3; ++i) {
    const uint64_t *s = c + i * MFX_DIP_PER_X;
    x[i]->distinct = s[MFX_DIP_DISTINCT]; x[i]->total = s[MFX_DIP_TOTAL]; x[i]->only_distinct = s[MFX_DIP_ONLY_DISTINCT];
    x[i]->only_total = s[MFX_DIP_ONLY_TOTAL]; x[i]->found = s[MFX_DIP_FOUND];
  }
  st->solid = c[MFX_DIP_SOLID]; st->n_read = c[MFX_DIP_N_READ]; st->n_shared = c[MFX_DIP_N_SHARED];
}

static int diploid_check_opts(const char *who, const mfx_db_join_opts *o, const uint64_t *asm_img, const uint64_t *cn_img, const uint64_t *n_entries,
                              const mfx_db_diploid_stats *st, const double *total64, const double *undrcpy64) {
  if (!o || !asm_img || !cn_img || !n_entries || !st) return mfx_fail(MFX_E_INVAL, "%s: null argument", who);
  if ((total64 != nullptr) != (undrcpy64 != nullptr)) return mfx_fail(MFX_E_INVAL, "%s: total64 and undrcpy64 are given together or not at all", who);
  if (total64 && o->n_prob && (!o->probK || !o->probP)) return mfx_fail(MFX_E_INVAL, "%s: null argument", who);
  if (o->copies < MFX_SPEC_MIN_COPIES || o->copies > MFX_SPEC_MAX_COPIES)      // (mfx_spectrum_run's bounds and texts)
    return mfx_fail(MFX_E_INVAL, "%s: copies = %u is outside [%u, %u]", who, o->copies, MFX_SPEC_MIN_COPIES, MFX_SPEC_MAX_COPIES);
  if (o->max_mult < MFX_SPEC_MIN_MULT || o->max_mult > MFX_SPEC_MAX_MULT)
    return mfx_fail(MFX_E_INVAL, "%s: max_mult = %u is outside [%u, %u]", who, o->max_mult, MFX_SPEC_MIN_MULT, MFX_SPEC_MAX_MULT);
  return MFX_OK;
}

static int db_diploid_impl(const char *read_path, const char *hap1_path, const char *hap2_path, const mfx_db_join_opts *o, uint64_t *asm_img, uint64_t *cn_img,
                           uint64_t *n_entries, mfx_db_diploid_stats *st, double *total64, double *undrcpy64) {
  const char *who = "mfx_db_diploid";
  const double t_begin = db_now();
  // ---- every check that needs no device
  if (!read_path || !hap1_path || !hap2_path) return mfx_fail(MFX_E_INVAL, "%s: null argument", who);
  if (int rc = diploid_check_opts(who, o, asm_img, cn_img, n_entries, st, total64, undrcpy64)) return rc;
  const bool pieces = total64 != nullptr;
  MergeIns ins;
  const char *paths[3] = {read_path, hap1_path, hap2_path};
  if (int rc = db_open_inputs(paths, 3, who, "the sorted join takes", "the inputs are of one k", ins)) return rc;
  const int k = (int)ins[0]->h.k;
  MergeWindows P;
  if (int rc = merge_plan_windows(ins, k, who, P)) return rc;
  uint64_t max_asm = 0;                                        // the most a window's blocks hold of the two assemblies together
  for (size_t w = 0; w < P.win.size(); ++w) {
    uint64_t a = 0;
    for (uint32_t i = 1; i < 3; ++i) a += mfx_merge_block_pairs(P.pin[i], P.blk[2 * (w * 3 + i)], P.blk[2 * (w * 3 + i) + 1]);
    max_asm = std::max(max_asm, a);
  }
  const uint64_t W = (uint64_t)o->max_mult + 1, cls_cells = MFX_DIP_ROWS * W, cn_cells = (uint64_t)(o->copies + 2u) * W;
  // res: [0] the k-mers of the reads and of an assembly, [1] spare; the class image and its counter word; the cn image and its counter word;
  // the 256 piece sums; the copies of the counters
  const size_t off_cls = 2, off_cn = off_cls + cls_cells + 1, off_sums = off_cn + cn_cells + 1, off_cnt = off_sums + 256, res_words = off_cnt + MFX_DIP_STAT_WORDS;
  std::vector<uint64_t> res(res_words, 0);
  DbPass pass(3);
  double t_pair = 0, t_join = 0;
  if (P.max_pairs) {
    DeviceBack back;
    MFX_HIP(hipSetDevice(o->device));
    // own.p[0]: one buffer of cap pairs, the k-mers in front of the counts: the decoded runs of the three inputs.  p[1]: the result.  p[2]: the pair
    // kernel's tile offsets.  p[3]: the tagged merged run of the two assemblies (acap pairs).  p[4]: the pair run (acap k-mers, acap words).
    // p[5], p[6]: the -prob table.
    const uint64_t cap = P.max_pairs + 1, acap = max_asm + 1, tiles = mfx_dip_tiles(max_asm), np = o->n_prob && pieces ? o->n_prob : 1;
    MergeDecoder dec;
    DbDev own;
    uint64_t total = 0;
    if (hipError_t e = db_alloc(dec, P, 3, own, {cap * 12, res_words * 8, (tiles + 1) * 8, acap * 12, acap * 16, np * sizeof(uint32_t), np * sizeof(double)}, &total))
      return mfx_fail(MFX_E_NOMEM, "%s: the buffers of a window of %lu pairs, %lu of them the assemblies' (%.3f GB) do not fit the device: %s; lower MFX_MERGE_RANGE", who,
                      (unsigned long)P.max_pairs, (unsigned long)max_asm, (double)total / 1e9, hipGetErrorString(e));
    uint64_t *d_keys = (uint64_t *)own.p[0], *d_res = (uint64_t *)own.p[1], *d_tile = (uint64_t *)own.p[2];
    uint32_t *d_vals = (uint32_t *)((char *)own.p[0] + cap * 8), *d_probK = (uint32_t *)own.p[5];
    uint64_t *m_keys = (uint64_t *)own.p[3], *p_keys = (uint64_t *)own.p[4], *p_vals = p_keys + acap;
    uint32_t *m_vals = (uint32_t *)((char *)own.p[3] + acap * 8);
    double *d_probP = (double *)own.p[6];
    MFX_HIP(mfx_memset_now(d_res, 0, res_words * 8));
    if (pieces && o->n_prob)
      if (int rc = db_upload_prob(o, d_probK, d_probP)) return rc;
    int grid = 1;                                                // the workgroups a CU holds at once (mfx_diploid.hip: LDS)
    if (int rc = db_grid(o->device, 2, &grid)) return rc;
    const mfx_spectrum_args cn = db_spectrum_args(o->copies, o->max_mult, mfx_dip_lds_cols(o->copies, o->max_mult), d_res + off_cn);
    mfx_spectrum_args cls = cn;
    cls.copies = MFX_DIP_ROWS - 2u;
    cls.img = d_res + off_cls;
    const bool timing = getenv("MFX_DB_TIMING") != nullptr;
    const int rc_pass = db_each_window(ins, P, k, who, dec, d_keys, d_vals, pass, [&](std::vector<MergeRun> &runs) -> int {
      double t0 = db_now();
      const MergeRun a = runs[0], h1 = runs[1], h2 = runs[2];
      // ---- a. the pair run: the role into the two low bits of the assemblies' k-mers, one merge, the head positions compacted
      const uint64_t M = h1.len + h2.len;
      uint64_t n_pairs = 0;
      if (M > max_asm) return mfx_fail(MFX_E_INVAL, "%s: a window does not match its plan", who);      // (nothing is merged beyond the buffers)
      if (M) {
        MFX_HIP(mfx_k_trio_tag(d_keys + h1.off, h1.len, MFX_DIP_HAP1, nullptr));
        MFX_HIP(mfx_k_trio_tag(d_keys + h2.off, h2.len, MFX_DIP_HAP2, nullptr));
        MFX_HIP(mfx_k_merge_pairs(d_keys + h1.off, d_vals + h1.off, h1.len, d_keys + h2.off, d_vals + h2.off, h2.len, m_keys, m_vals, nullptr));
        MFX_HIP(mfx_k_dip_pairs(m_keys, m_vals, M, d_tile, p_keys, p_vals, nullptr));
        MFX_HIP(hipMemcpyAsync(&n_pairs, d_tile + mfx_dip_tiles(M), 8, hipMemcpyDeviceToHost, nullptr));
        MFX_HIP(hipStreamSynchronize(nullptr));
      }
      if (n_pairs > M || 2 * n_pairs < M) return mfx_fail(MFX_E_HIP, "%s: the pair run of a window is damaged", who);
      double t1 = db_now();
      t_pair += t1 - t0;
      // ---- b. the join of the read run against it
      MFX_HIP(mfx_k_dip_join(d_keys + a.off, d_vals + a.off, a.len, p_keys, p_vals, n_pairs, cls, cn, o->minV, o->maxV, k, pieces ? 1 : 0, o->peak,
                             pieces ? o->n_prob : 0u, d_probK, d_probP, reinterpret_cast<double *>(d_res + off_sums), d_res + off_cnt, d_res, grid, nullptr));
      if (timing) MFX_HIP(hipStreamSynchronize(nullptr));
      t_join += db_now() - t1;
      return MFX_OK;
    });
    if (rc_pass) return rc_pass;
    MFX_HIP(hipMemcpy(res.data(), d_res, res_words * 8, hipMemcpyDeviceToHost));
  }
  // ---- what the windows held against what the files say, the counters against the files, the images against their counters: no partial result
  if (int rc = pass.check(ins)) return rc;
  const std::vector<uint64_t> &got = pass.got;
  uint64_t c[MFX_DIP_NSTATS];
  for (uint32_t s = 0; s < MFX_DIP_NSTATS; ++s) {
    c[s] = 0;
    for (uint32_t j = 0; j < MFX_DIP_STAT_SHARDS; ++j) c[s] += res[off_cnt + j * MFX_DIP_STAT_STRIDE + s];
  }
  const uint64_t d1 = c[MFX_DIP_DISTINCT], d2 = c[MFX_DIP_PER_X + MFX_DIP_DISTINCT], db = c[2 * MFX_DIP_PER_X + MFX_DIP_DISTINCT];
  if (d1 != got[1] || d2 != got[2] || c[MFX_DIP_N_READ] != got[0] || d1 + d2 - c[MFX_DIP_N_SHARED] != db ||
      res[0] != db - c[2 * MFX_DIP_PER_X + MFX_DIP_ONLY_DISTINCT])
    return mfx_fail(MFX_E_HIP, "%s: the join counted %lu, %lu and %lu k-mers of the reads, hap1 and hap2 (%lu shared, %lu of either, %lu of the reads and an assembly): "
                    "not what databases of %lu, %lu and %lu k-mers give", who, (unsigned long)c[MFX_DIP_N_READ], (unsigned long)d1, (unsigned long)d2,
                    (unsigned long)c[MFX_DIP_N_SHARED], (unsigned long)db, (unsigned long)res[0], (unsigned long)got[0], (unsigned long)got[1], (unsigned long)got[2]);
  uint64_t sum_cls = 0, sum_cn = 0;
  for (size_t i = 0; i < cls_cells; ++i) sum_cls += res[off_cls + i];
  for (size_t i = 0; i < cn_cells; ++i) sum_cn += res[off_cn + i];
  if (sum_cls != res[off_cls + cls_cells] || sum_cn != res[off_cn + cn_cells] || sum_cls != sum_cn)
    return mfx_fail(MFX_E_HIP, "%s: the images sum to %lu and %lu, the join counted %lu and %lu entries", who, (unsigned long)sum_cls, (unsigned long)sum_cn,
                    (unsigned long)res[off_cls + cls_cells], (unsigned long)res[off_cn + cn_cells]);
  const bool filtered = o->minV > 1 || o->maxV < 0xffffffffull;      // (a count is 1 at the least: no other filter makes an entry vanish)
  if (!filtered && sum_cn != got[0] + db - res[0])
    return mfx_fail(MFX_E_HIP, "%s: the join counted %lu entries, the inputs hold %lu distinct k-mers", who, (unsigned long)sum_cn, (unsigned long)(got[0] + db - res[0]));
  memcpy(asm_img, res.data() + off_cls, cls_cells * 8);
  memcpy(cn_img, res.data() + off_cn, cn_cells * 8);
  *n_entries = sum_cn;
  if (pieces) {
    memcpy(total64, res.data() + off_sums, 64 * sizeof(double));
    memcpy(undrcpy64, res.data() + off_sums + 64, 3 * 64 * sizeof(double));
  }
  memset(st, 0, sizeof(*st));
  diploid_fill_stats(c, st);
  st->n_hap1 = got[1]; st->n_hap2 = got[2]; st->windows = pass.windows;
  st->t_read = pass.t_read; st->t_decode = pass.t_decode; st->t_pair = t_pair; st->t_join = t_join; st->t_total = db_now() - t_begin;
  return MFX_OK;
}

extern "C" int mfx_db_diploid(const char *read_path, const char *hap1_path, const char *hap2_path, const mfx_db_join_opts *o, uint64_t *asm_img, uint64_t *cn_img,
                              uint64_t *n_entries, mfx_db_diploid_stats *st, double *total64, double *undrcpy64) {
  return db_guard("mfx_db_diploid", [&] { return db_diploid_impl(read_path, hap1_path, hap2_path, o, asm_img, cn_img, n_entries, st, total64, undrcpy64); });
}

extern "C" int mfx_db_diploid_host(const uint64_t *read_keys, const uint32_t *read_vals, uint64_t n_read, const uint64_t *hap1_keys, const uint32_t *hap1_vals,
                                   uint64_t n_hap1, const uint64_t *hap2_keys, const uint32_t *hap2_vals, uint64_t n_hap2, int k, const mfx_db_join_opts *o, uint64_t *keys,
                                   uint32_t *readV, uint32_t *c1V, uint32_t *c2V, uint64_t cap, uint64_t *n_kmers, uint64_t *asm_img, uint64_t *cn_img, uint64_t *n_entries,
                                   mfx_db_diploid_stats *st, double *total64, double *undrcpy64) {
  const char *who = "mfx_db_diploid_host";
  if ((n_read && (!read_keys || !read_vals)) || (n_hap1 && (!hap1_keys || !hap1_vals)) || (n_hap2 && (!hap2_keys || !hap2_vals)) || !n_kmers ||
      (cap && (!keys || !readV || !c1V || !c2V)))
    return mfx_fail(MFX_E_INVAL, "%s: null argument", who);
  if (int rc = diploid_check_opts(who, o, asm_img, cn_img, n_entries, st, total64, undrcpy64)) return rc;
  if (k < 1 || k > MFX_MAX_K_NARROW) return mfx_fail(MFX_E_INVAL, "%s: k = %d is outside [1, %d]", who, k, MFX_MAX_K_NARROW);
  return db_guard(who, [&]() -> int {
    mfx_dip_host_result R;
    uint64_t n = 0;
    mfx_dip_host(read_keys, read_vals, n_read, hap1_keys, hap1_vals, n_hap1, hap2_keys, hap2_vals, n_hap2, k, o->minV, o->maxV, o->copies, o->max_mult, total64 != nullptr,
                 [&](uint32_t r) { double rk, pr; mfx_getK_core(o->peak, o->n_prob, o->probK, o->probP, r, rk, pr); return rk; },
                 [&](uint64_t key, uint32_t r, uint32_t c1, uint32_t c2) {
                   if (n < cap) { keys[n] = key; readV[n] = r; c1V[n] = c1; c2V[n] = c2; }
                   ++n;
                 }, R);
    if (R.stats[MFX_DIP_DISTINCT] != n_hap1 || R.stats[MFX_DIP_PER_X + MFX_DIP_DISTINCT] != n_hap2 || R.stats[MFX_DIP_N_READ] != n_read)
      return mfx_fail(MFX_E_INVAL, "%s: the runs do not ascend strictly, or hold a count of 0", who);
    *n_kmers = n;
    memcpy(asm_img, R.asm_img.data(), R.asm_img.size() * 8);
    memcpy(cn_img, R.cn_img.data(), R.cn_img.size() * 8);
    *n_entries = R.n_entries;
    if (total64) { memcpy(total64, R.tot, sizeof(R.tot)); memcpy(undrcpy64, R.und, sizeof(R.und)); }
    memset(st, 0, sizeof(*st));
    diploid_fill_stats(R.stats, st);
    st->n_hap1 = n_hap1; st->n_hap2 = n_hap2;
    return MFX_OK;
  });
}

extern "C" int mfx_diploid_write_asm(const uint64_t *img, uint32_t max_mult, const char *path) {
  if (!img || !path) return mfx_fail(MFX_E_INVAL, "mfx_diploid_write_asm: null argument");
  if (max_mult < MFX_SPEC_MIN_MULT || max_mult > MFX_SPEC_MAX_MULT)
    return mfx_fail(MFX_E_INVAL, "mfx_diploid_write_asm: max_mult = %u is outside [%u, %u]", max_mult, MFX_SPEC_MIN_MULT, MFX_SPEC_MAX_MULT);
  static const char *const label[MFX_DIP_ROWS] = {"read-only", "hap1-only", "hap2-only", "shared"};
  mfx_file fh = mfx_open_writer(path, false);                    // compressor chosen by suffix (mfx_pipe.h)
  if (!fh.f) return mfx_fail(MFX_E_IO, "mfx_diploid_write_asm: cannot open '%s' for writing", path);
  fprintf(fh.f, "Assembly\tkmer_multiplicity\tCount\n");
  for (uint32_t r = 0; r < MFX_DIP_ROWS; ++r)
    for (uint32_t m = 0; m <= max_mult; ++m)
      if (img[(size_t)r * (max_mult + 1u) + m]) fprintf(fh.f, "%s\t%u\t%llu\n", label[r], m, (unsigned long long)img[(size_t)r * (max_mult + 1u) + m]);
  if (mfx_close(fh)) return mfx_fail(MFX_E_IO, "mfx_diploid_write_asm: writing '%s' failed", path);
  return MFX_OK;
}
