// mfx_db_windows.cpp -- the window session of the sorted-database calls (mfx_db_windows.h): the inputs, the windows, a window's way from the
// files to dense runs on the device, the merge tree, the closing check.  file blocks -> ascending runs on the device; no table in between.
#include "mfx_db_windows.h"

#include <fcntl.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

static_assert(MFX_MERGE_BLOCK == MFX_DELTA_BLOCK, "mfx_merge.h plans in blocks of the delta form");

int merge_open_input(const char *path, MergeIn &in, const char *who) {
  in.path = path;
  const int fmt = detect(in.path);
  if (!fmt) return mfx_fail(MFX_E_IO, "%s: the input '%s' does not exist", who, path);
  if (fmt == MFX_DB_MERYL) return mfx_fail(MFX_E_FORMAT, "%s: '%s' is a meryl directory; the inputs are sorted flat databases: run `merfin -convert` first", who, path);
  if (fmt == MFX_DB_TEXT) return mfx_fail(MFX_E_FORMAT, "%s: '%s' is not a flat k-mer file (`meryl print` text?); the inputs are sorted flat databases: run `merfin -convert` first", who, path);
  in.fd = open(path, O_RDONLY | O_CLOEXEC);
  struct stat st;
  if (in.fd < 0 || fstat(in.fd, &st) != 0) return mfx_fail(MFX_E_IO, "cannot open '%s'", path);
  const uint64_t fsize = (uint64_t)st.st_size;
  if (fsize < sizeof(in.h) || pread(in.fd, &in.h, sizeof(in.h), 0) != (ssize_t)sizeof(in.h)) return mfx_fail(MFX_E_FORMAT, "'%s': truncated header", path);
  if (const char *why = flat_header_problem(in.h, fsize)) return mfx_fail(MFX_E_FORMAT, "'%s': %s", path, why);
  if (in.h.flags & FLAT_PLACED)
    return mfx_fail(MFX_E_FORMAT, "%s: '%s' is a placed database; the inputs are sorted by k-mer: merge those, then place the result (merfin -convert -placed)", who, path);
  if (in.h.n == 0) return MFX_OK;                               // (no k-mers: what mfx_db_write_flat writes for none has no blocks in any form)
  if (!(in.h.flags & FLAT_DELTA))
    return mfx_fail(MFX_E_FORMAT, "%s: '%s' is a %s flat file, not a sorted one: run `merfin -convert` first", who, path, (in.h.flags & FLAT_PACKED) ? "packed" : "plain");
  uint64_t expect = 0;
  if (int rc = read_delta_directory(in.fd, path, in.h, fsize, in.dir, &in.nblocks, &expect)) return rc;
  const uint64_t ne = in.h.n_escape;
  try { in.ek.resize(ne); in.ev.resize(ne); }
  catch (const std::exception &) { return mfx_fail(MFX_E_NOMEM, "'%s': no memory for %lu escapes", path, (unsigned long)ne); }
  if (ne && (pread(in.fd, in.ek.data(), ne * 8, (off_t)expect) != (ssize_t)(ne * 8) || pread(in.fd, in.ev.data(), ne * 4, (off_t)(expect + ne * 8)) != (ssize_t)(ne * 4)))
    return mfx_fail(MFX_E_IO, "reading '%s' failed", path);
  for (uint64_t i = 0; i < ne; ++i) {
    if (!flat_key_fits(in.ek[i], in.h.k)) return mfx_fail(MFX_E_FORMAT, "'%s': an escaped k-mer is wider than 2k bits", path);
    if (i && in.ek[i] <= in.ek[i - 1]) return mfx_fail(MFX_E_FORMAT, "'%s': the escape list of a sorted database does not ascend", path);
  }
  return MFX_OK;
}

int db_open_inputs(const char *const *paths, uint32_t n, const char *who, const char *wide, const char *one_k, MergeIns &ins) {
  for (uint32_t i = 0; i < n; ++i) {
    if (!paths[i]) return mfx_fail(MFX_E_INVAL, "%s: null argument", who);
    mfx_db_info info;                                            // (k > 31 has no sorted form: said as that, not as "a plain flat file")
    if (wide && detect(paths[i]) == MFX_DB_FLAT && mfx_db_probe_impl(paths[i], &info) == MFX_OK && info.k > MFX_MAX_K_NARROW)
      return mfx_fail(MFX_E_INVAL, "%s: '%s' holds %d-mers: %s k <= %d", who, paths[i], info.k, wide, MFX_MAX_K_NARROW);
    ins.emplace_back(new MergeIn);
    if (int rc = merge_open_input(paths[i], *ins.back(), who)) return rc;
    if (ins.back()->h.k != ins[0]->h.k)
      return mfx_fail(MFX_E_INVAL, "%s: '%s' holds %u-mers, '%s' %u-mers: %s", who, paths[i], ins.back()->h.k, ins[0]->path.c_str(), ins[0]->h.k, one_k);
  }
  return MFX_OK;
}

int db_output_is_input(const char *out_path, const MergeIns &ins, size_t from) {
  struct stat so, si;
  if (stat(out_path, &so) != 0) return -1;
  for (size_t i = from; i < ins.size(); ++i)
    if (fstat(ins[i]->fd, &si) == 0 && si.st_dev == so.st_dev && si.st_ino == so.st_ino) return (int)i;
  return -1;
}

static uint64_t merge_range_knob() {
  uint64_t R = MFX_MERGE_RANGE_DEFAULT;
  if (const char *e = getenv("MFX_MERGE_RANGE")) {             // read per call: tests reach many windows on small files
    const long long v = atoll(e);
    if (v > 0 && (uint64_t)v < R) R = (uint64_t)v;
  }
  return R;
}

int merge_plan_windows(const MergeIns &ins, int k, const char *who, MergeWindows &P) {
  const uint32_t n_in = (uint32_t)ins.size();
  P.pin.resize(n_in);
  for (uint32_t i = 0; i < n_in; ++i) { P.pin[i] = mfx_merge_input{ins[i]->dir.data(), 2u, ins[i]->nblocks, ins[i]->h.n}; P.n_all += ins[i]->h.n; }
  mfx_merge_plan(P.pin.data(), n_in, k, merge_range_knob(), P.win, P.blk);
  for (size_t w = 0; w < P.win.size(); ++w) {
    uint64_t bytes = 0, tasks = 0, esc = 0;
    for (uint32_t i = 0; i < n_in; ++i) {
      const uint64_t b0 = P.blk[2 * (w * n_in + i)], b1 = P.blk[2 * (w * n_in + i) + 1];
      if (b1 <= b0) continue;
      bytes += ins[i]->off(b1) - ins[i]->off(b0);
      tasks += b1 - b0;
      uint64_t e0, e1;
      mfx_merge_escape_slice(ins[i]->ek.data(), ins[i]->ek.size(), P.win[w].lo, P.win[w].hi, &e0, &e1);
      esc += e1 - e0;
    }
    P.max_pairs = std::max(P.max_pairs, P.win[w].pairs); P.max_bytes = std::max(P.max_bytes, bytes);
    P.max_tasks = std::max(P.max_tasks, tasks); P.max_esc = std::max(P.max_esc, esc);
  }
  if (P.max_pairs > 0x7fffffffull || P.max_esc > 0x7fffffffull)
    return mfx_fail(MFX_E_INVAL, "%s: a window of %lu pairs (at most 2^31 - 1); lower MFX_MERGE_RANGE", who, (unsigned long)P.max_pairs);
  return MFX_OK;
}

hipError_t MergeDecoder::init(const MergeWindows &P, uint32_t n_in) {
  // dev.p[0]: the window's blocks.  p[1]: tasks, their below / above, the inputs' error words.  p[2], p[3]: the window's escapes.
  const uint64_t size[4] = {P.max_bytes + 8, P.max_tasks * (sizeof(mfx_merge_task) + 8) + n_in * 4, (P.max_esc + 1) * 8, (P.max_esc + 1) * 4};
  bytes = size[0] + size[1] + size[2] + size[3];
  for (int i = 0; i < 4; ++i)
    if (hipError_t e = hipMalloc(&dev.p[i], size[i])) return e;
  d_words = dev.p[0];
  d_tasks = (mfx_merge_task *)dev.p[1];
  d_below = (uint32_t *)(d_tasks + P.max_tasks); d_above = d_below + P.max_tasks; d_err = d_above + P.max_tasks;
  d_ek = (uint64_t *)dev.p[2]; d_ev = (uint32_t *)dev.p[3];
  return hipHostMalloc(&pinned, P.max_bytes + 8, hipHostMallocDefault);
}

hipError_t db_alloc(MergeDecoder &dec, const MergeWindows &P, uint32_t n_in, DbDev &own, std::initializer_list<uint64_t> sizes, uint64_t *total) {
  hipError_t e = dec.init(P, n_in);
  *total = dec.device_bytes();
  int i = 0;
  for (uint64_t s : sizes) {
    if (e == hipSuccess && s) e = hipMalloc(&own.p[i], s);
    *total += s;
    ++i;
  }
  if (e != hipSuccess) (void)hipGetLastError();
  return e;
}

int merge_decode_window(const MergeIns &ins, const MergeWindows &P, size_t wi, int k, const char *who, MergeDecoder &D, uint64_t *keys, uint32_t *vals) {
  const uint32_t n_in = (uint32_t)ins.size();
  const uint64_t lo = P.win[wi].lo, hi = P.win[wi].hi, END = mfx_merge_end(k);
  uint64_t *words = (uint64_t *)D.pinned;
  D.run_off.resize(n_in); D.run_len.resize(n_in); D.first_task.resize(n_in); D.errs.resize(n_in);
  D.t_read = D.t_decode = 0;
  double t0 = db_now();
  // ---- the window's blocks and escapes, input after input
  D.tasks.clear(); D.hek.clear(); D.hev.clear();
  uint64_t nwords = 0, npairs = 0;
  for (uint32_t i = 0; i < n_in; ++i) {
    const MergeIn &in = *ins[i];
    const uint64_t b0 = P.blk[2 * (wi * n_in + i)], b1 = P.blk[2 * (wi * n_in + i) + 1];
    D.run_off[i] = npairs; D.run_len[i] = 0; D.first_task[i] = D.tasks.size();
    if (b1 <= b0) continue;
    const uint64_t from = in.off(b0), bytes = in.off(b1) - from;
    if ((nwords * 8 + bytes) > P.max_bytes) return mfx_fail(MFX_E_INVAL, "%s: a window does not match its plan", who);      // (nothing is read beyond the buffer)
    for (uint64_t got = 0; got < bytes;) {
      const ssize_t r = pread(in.fd, (char *)(words + nwords) + got, bytes - got, (off_t)(from + got));
      if (r <= 0) return mfx_fail(MFX_E_IO, "reading '%s' failed", in.path.c_str());
      got += (uint64_t)r;
    }
    uint64_t e0, e1;
    mfx_merge_escape_slice(in.ek.data(), in.ek.size(), lo, hi, &e0, &e1);
    const uint32_t esc_lo = (uint32_t)D.hek.size(), esc_hi = esc_lo + (uint32_t)(e1 - e0);
    D.hek.insert(D.hek.end(), in.ek.begin() + e0, in.ek.begin() + e1);
    D.hev.insert(D.hev.end(), in.ev.begin() + e0, in.ev.begin() + e1);
    for (uint64_t b = b0; b < b1; ++b) {
      mfx_merge_task t;
      t.word_off = nwords + (in.off(b) - from) / 8;
      t.first = in.dir[2 * b];
      t.limit = b + 1 < in.nblocks ? in.dir[2 * (b + 1)] : END;
      t.out = npairs + (b - b0) * MFX_DELTA_BLOCK;
      t.kb = (uint32_t)(in.dir[2 * b + 1] >> 48) & 0xffu;
      t.vb = (uint32_t)(in.dir[2 * b + 1] >> 56) & 0xffu;
      t.cnt = (uint32_t)std::min<uint64_t>(MFX_DELTA_BLOCK, in.h.n - b * MFX_DELTA_BLOCK);
      t.esc_lo = esc_lo; t.esc_hi = esc_hi; t.input = i;
      D.tasks.push_back(t);
    }
    D.run_len[i] = mfx_merge_block_pairs(P.pin[i], b0, b1);
    npairs += D.run_len[i];
    nwords += bytes / 8;
  }
  const uint32_t nt = (uint32_t)D.tasks.size();
  if (npairs != P.win[wi].pairs || npairs > P.max_pairs || nwords * 8 > P.max_bytes || nt > P.max_tasks || D.hek.size() > P.max_esc)
    return mfx_fail(MFX_E_INVAL, "%s: a window does not match its plan", who);      // (nothing is decoded beyond the buffers)
  MFX_HIP(hipMemcpyAsync(D.d_words, words, nwords * 8, hipMemcpyHostToDevice, nullptr));
  MFX_HIP(hipMemcpyAsync(D.d_tasks, D.tasks.data(), nt * sizeof(mfx_merge_task), hipMemcpyHostToDevice, nullptr));
  if (!D.hek.empty()) {
    MFX_HIP(hipMemcpyAsync(D.d_ek, D.hek.data(), D.hek.size() * 8, hipMemcpyHostToDevice, nullptr));
    MFX_HIP(hipMemcpyAsync(D.d_ev, D.hev.data(), D.hev.size() * 4, hipMemcpyHostToDevice, nullptr));
  }
  MFX_HIP(hipMemsetAsync(D.d_err, 0, n_in * 4, nullptr));
  MFX_HIP(hipStreamSynchronize(nullptr));                      // (the host arrays are filled again for the next window)
  double t1 = db_now();
  D.t_read = t1 - t0;
  // ---- decode: one ascending run per input
  MFX_HIP(mfx_k_delta_decode(D.d_tasks, nt, (const uint64_t *)D.d_words, D.d_ek, D.d_ev, lo, hi, keys, vals, D.d_below, D.d_above, D.d_err, nullptr, D.zero_from));
  D.cnt.resize(2 * (size_t)nt);
  MFX_HIP(hipMemcpyAsync(D.cnt.data(), D.d_below, nt * 4, hipMemcpyDeviceToHost, nullptr));
  MFX_HIP(hipMemcpyAsync(D.cnt.data() + nt, D.d_above, nt * 4, hipMemcpyDeviceToHost, nullptr));
  MFX_HIP(hipMemcpyAsync(D.errs.data(), D.d_err, n_in * 4, hipMemcpyDeviceToHost, nullptr));
  MFX_HIP(hipStreamSynchronize(nullptr));
  D.t_decode = db_now() - t1;
  for (uint32_t i = 0; i < n_in; ++i)
    if (D.errs[i])
      return mfx_fail(MFX_E_FORMAT, "'%s': a block holds what no writer makes (%s%s%s): the file is damaged", ins[i]->path.c_str(),
                      (D.errs[i] & MFX_MERGE_ERR_ORDER) ? "k-mers that do not ascend below the next block's first; " : "",
                      (D.errs[i] & MFX_MERGE_ERR_ESCAPE) ? "an escaped count that is not in the escape list; " : "", (D.errs[i] & MFX_MERGE_ERR_ZERO) ? "a count of zero; " : "");
  D.runs.clear();
  for (uint32_t i = 0; i < n_in; ++i) {
    const uint64_t f = D.first_task[i], l = (i + 1 < n_in ? D.first_task[i + 1] : nt);
    MergeRun r{0, 0};
    // (ascending k-mers below every block's limit: only an input's first block reaches under lo, only its last to hi and beyond)
    if (!mfx_join_trim(D.run_off[i], D.run_len[i], D.cnt.data() + f, D.cnt.data() + nt + f, l - f, &r.off, &r.len))
      return mfx_fail(MFX_E_FORMAT, "'%s': the k-mers of a block lie outside its place in the directory", ins[i]->path.c_str());
    D.runs.push_back(r);
  }
  return MFX_OK;
}

int merge_tree(std::vector<MergeRun> &runs, uint64_t *const bk[2], uint32_t *const bv[2], int &cur) {
  std::vector<MergeRun> next;
  while (runs.size() > 1) {
    next.clear();
    uint64_t at = 0;
    for (size_t j = 0; j < runs.size(); j += 2) {
      const MergeRun a = runs[j], b = j + 1 < runs.size() ? runs[j + 1] : MergeRun{0, 0};
      MFX_HIP(mfx_k_merge_pairs(bk[cur] + a.off, bv[cur] + a.off, a.len, bk[cur] + b.off, bv[cur] + b.off, b.len, bk[cur ^ 1] + at, bv[cur ^ 1] + at, nullptr));
      next.push_back(MergeRun{at, a.len + b.len});
      at += a.len + b.len;
    }
    runs.swap(next);
    cur ^= 1;
  }
  return MFX_OK;
}

int DbPass::check(const MergeIns &ins) const {
  for (size_t i = 0; i < ins.size(); ++i)
    if (got[i] != ins[i]->h.n)
      return mfx_fail(MFX_E_FORMAT, "'%s': the windows hold %lu of its %lu k-mers: the directory does not describe the blocks", ins[i]->path.c_str(), (unsigned long)got[i],
                      (unsigned long)ins[i]->h.n);
  return MFX_OK;
}

mfx_spectrum_args db_spectrum_args(uint32_t copies, uint32_t max_mult, uint32_t lds_cols, uint64_t *img) {
  mfx_spectrum_args sa{};
  sa.copies = copies;
  sa.max_mult = max_mult;
  sa.lds_cols = lds_cols;
  const char *ag = getenv("MFX_SPECTRUM_AGG");
  sa.aggregate = ag ? (atoi(ag) != 0) : MFX_SPEC_AGG_DEFAULT;
  sa.img = img;
  return sa;
}

int db_upload_prob(const mfx_db_join_opts *o, uint32_t *d_K, double *d_P) {
  MFX_HIP(hipMemcpy(d_K, o->probK, o->n_prob * sizeof(uint32_t), hipMemcpyHostToDevice));
  MFX_HIP(hipMemcpy(d_P, o->probP, o->n_prob * sizeof(double), hipMemcpyHostToDevice));
  return MFX_OK;
}

int db_grid(int device, int per_cu, int *grid) {
  int cus = 0;
  MFX_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  *grid = (cus > 0 ? cus : 256) * per_cu;
  return MFX_OK;
}
