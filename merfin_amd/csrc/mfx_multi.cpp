// mfx_multi.cpp -- -hist over several SLOTS (devices, or contexts on one) driven by ONE process (the reference is one binary
// driving all its workers, merfin.C:366-414): replicas of the index and of the assembly, the block-cyclic and the streamed run over
// them, parts of an assembly on sequence-only indexes, the sharded index and its router.  Every driver checks its slots
// (check_slots), adds their counts images (~1 MB each) on the host in slot order (mfx_histsum.h) -- integers exactly, koverCpy by
// the driver's own fixed order of fp64 operations, so the result is bit-stable run to run -- and ends in finish(), which folds
// the K* bins beyond the dense image in from every evaluator's overflow list.
#include "mfx_host.h"
#include "mfx_histsum.h"
#include "mfx_kernels.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <functional>
#include <thread>

// Doubling tree over the devices of a node: holder 0 has the data; in every round each holder feeds ONE device that does
// not have it yet, all copies of a round in flight together (xGMI is point to point: 1, 2, 4 source devices work in
// parallel, 7 replicas of a 97 GB table take 3 rounds instead of 7 copies through device 0's links one after the other).
// dev[h], ptr[h][s]: device and buffers of holder h; bytes[s]: size of segment s (the same for every holder).
static int tree_copy(const std::vector<int> &dev, const std::vector<std::vector<void *>> &ptr, const std::vector<size_t> &bytes) {
  const size_t H = dev.size();
  std::vector<hipStream_t> st(H, nullptr);
  int rc = MFX_OK;
  std::vector<size_t> have(1, 0);
  size_t next = 1;
  const size_t CH = 1ull << 30;
  while (next < H && rc == MFX_OK) {
    std::vector<size_t> fresh;
    for (size_t j = 0; j < have.size() && next < H && rc == MFX_OK; ++j, ++next) {
      const size_t from = have[j], to = next;
      DevGuard g(dev[to]);
      if (dev[from] != dev[to]) {
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, dev[to], dev[from]) == hipSuccess && can && hipDeviceEnablePeerAccess(dev[from], 0) != hipSuccess)
          (void)hipGetLastError();                              // "already enabled" is fine
      }
      hipError_t e = st[to] ? hipSuccess : hipStreamCreateWithFlags(&st[to], hipStreamNonBlocking);
      for (size_t sgi = 0; sgi < bytes.size() && e == hipSuccess; ++sgi)
        for (size_t o = 0; o < bytes[sgi] && e == hipSuccess; o += CH)
          e = hipMemcpyPeerAsync((char *)ptr[to][sgi] + o, dev[to], (const char *)ptr[from][sgi] + o, dev[from], std::min(CH, bytes[sgi] - o), st[to]);
      if (e != hipSuccess) rc = mfx_fail(MFX_E_HIP, "peer copy from device %d to device %d failed: %s", dev[from], dev[to], hipGetErrorString(e));
      fresh.push_back(to);
    }
    for (size_t t : fresh) {
      DevGuard g(dev[t]);
      const hipError_t e = st[t] ? hipStreamSynchronize(st[t]) : hipSuccess;
      if (e != hipSuccess && rc == MFX_OK) rc = mfx_fail(MFX_E_HIP, "peer copy to device %d failed: %s", dev[t], hipGetErrorString(e));
      have.push_back(t);
    }
  }
  for (size_t h = 0; h < H; ++h)
    if (st[h]) { DevGuard g(dev[h]); (void)hipStreamDestroy(st[h]); }
  return rc;
}

extern "C" int mfx_index_replicate_many(const mfx_index *src, const int *devices, uint32_t n, mfx_index **out) {
  if (!src || !devices || !out || n == 0) return mfx_fail(MFX_E_INVAL, "mfx_index_replicate_many: null argument");
  for (uint32_t i = 0; i < n; ++i) {
    out[i] = nullptr;
    if (devices[i] < 0 || devices[i] >= mfx_device_count()) return mfx_fail(MFX_E_INVAL, "mfx_index_replicate_many: device %d of %d", devices[i], mfx_device_count());
  }
  uint8_t hdr[MFX_INDEX_HEADER_BYTES];
  int rc = mfx_index_image_header(src, hdr);
  if (rc) return rc;
  std::vector<int> dev(1, src->device);
  std::vector<std::vector<void *>> ptr(1, std::vector<void *>{src->d_slots, src->d_meta});
  for (uint32_t i = 0; i < n && rc == MFX_OK; ++i) {
    out[i] = mfx_index_create_from_header(hdr, 0.0, devices[i]);
    if (!out[i]) { rc = mfx_last_error_code() ? mfx_last_error_code() : MFX_E_NOMEM; break; }
    dev.push_back(devices[i]);
    ptr.push_back(std::vector<void *>{out[i]->d_slots, out[i]->d_meta});
  }
  if (rc == MFX_OK) {
    { DevGuard g(src->device); (void)hipDeviceSynchronize(); }          // the source's last inserts are done
    rc = tree_copy(dev, ptr, std::vector<size_t>{(size_t)(src->total_lines() * MFX_ALIGN), 4 * sizeof(uint64_t)});
  }
  if (rc != MFX_OK) {
    const std::string why = mfx_last_error();
    for (uint32_t i = 0; i < n; ++i) { if (out[i]) mfx_index_free(out[i]); out[i] = nullptr; }
    return mfx_fail(rc, "copying the k-mer table to %u device(s) failed: %s", n, why.c_str());
  }
  for (uint32_t i = 0; i < n; ++i) {
    out[i]->fingerprint = src->fingerprint;
    out[i]->seq_digest = src->seq_digest;
    (void)mfx_index_commit(out[i]);
  }
  return MFX_OK;
}

extern "C" mfx_index *mfx_index_replicate(const mfx_index *src, int device) {
  mfx_index *out = nullptr;
  return mfx_index_replicate_many(src, &device, 1, &out) == MFX_OK ? out : nullptr;
}


// The assembly travels between devices as its packed planes (0.375 B per base instead of 1); a replica holds the planes
// only and unpacks them if a kernel asks for one byte per base (mfx_seq_ensure_ascii).
extern "C" int mfx_seq_replicate_many(const mfx_seq *csrc, const int *devices, uint32_t n, mfx_seq **out) {
  if (!csrc || !devices || !out || n == 0) return mfx_fail(MFX_E_INVAL, "mfx_seq_replicate_many: null argument");
  for (uint32_t i = 0; i < n; ++i) {
    out[i] = nullptr;
    if (devices[i] < 0 || devices[i] >= mfx_device_count()) return mfx_fail(MFX_E_INVAL, "mfx_seq_replicate_many: device %d of %d", devices[i], mfx_device_count());
  }
  mfx_seq *src = const_cast<mfx_seq *>(csrc);
  if (src->partial) return mfx_seq_partial_error(src, "mfx_seq_replicate");
  int rc = mfx_seq_pack(src);
  if (rc) return rc;
  const uint64_t pw = seq_plane_words(src);
  std::vector<int> dev(1, src->device);
  std::vector<std::vector<void *>> ptr(1, std::vector<void *>{src->d_codes, src->d_valid});
  for (uint32_t i = 0; i < n && rc == MFX_OK; ++i) {
    out[i] = mfx_seq_create(devices[i], src->len.data(), src->ncontigs);
    if (!out[i]) { rc = mfx_last_error_code() ? mfx_last_error_code() : MFX_E_NOMEM; break; }
    DevGuard g(devices[i]);
    rc = seq_alloc_planes(out[i]);
    dev.push_back(devices[i]);
    ptr.push_back(std::vector<void *>{out[i]->d_codes, out[i]->d_valid});
  }
  if (rc == MFX_OK) {
    { DevGuard g(devices[n - 1]); (void)hipDeviceSynchronize(); }       // the memsets of the last replica's planes
    for (uint32_t i = 0; i + 1 < n; ++i) { DevGuard g(devices[i]); (void)hipDeviceSynchronize(); }
    rc = tree_copy(dev, ptr, std::vector<size_t>{(size_t)(pw * sizeof(uint64_t)), (size_t)(pw * sizeof(uint32_t))});
  }
  if (rc != MFX_OK) {
    const std::string why = mfx_last_error();
    for (uint32_t i = 0; i < n; ++i) { if (out[i]) mfx_seq_free(out[i]); out[i] = nullptr; }
    return mfx_fail(rc, "copying the packed assembly to %u device(s) failed: %s", n, why.c_str());
  }
  for (uint32_t i = 0; i < n; ++i) { out[i]->bases_stale = true; out[i]->planes_ok = true; }
  return MFX_OK;
}

extern "C" mfx_seq *mfx_seq_replicate(const mfx_seq *src, int device) {
  mfx_seq *out = nullptr;
  return mfx_seq_replicate_many(src, &device, 1, &out) == MFX_OK ? out : nullptr;
}

// The rules a driver asks of its slots besides the ones every driver has (no null object, evaluator and sequence of a slot on one
// device, the same bins everywhere):
enum : unsigned { SAME_NTILES = 1, SAME_NCONTIGS = 2, SAME_LEN = 4, DISTINCT_EVALS = 8, DISTINCT_SEQS = 16, NOT_WIDE = 32 };

static int check_slots(const char *who, mfx_eval *const *evs, const mfx_seq *const *seqs, uint32_t ndev, unsigned flags) {
  for (uint32_t d = 0; d < ndev; ++d) {
    if (!evs[d] || !seqs[d]) return mfx_fail(MFX_E_INVAL, "%s: null evaluator / sequence for slot %u", who, d);
    if (evs[d]->device != seqs[d]->device) return mfx_fail(MFX_E_INVAL, "slot %u: evaluator and sequence live on different devices", d);
    if (evs[d]->nbins != evs[0]->nbins) return mfx_fail(MFX_E_INVAL, "slot %u: the evaluators of one run must have the same bins", d);
    if (((flags & SAME_NTILES) && seqs[d]->ntiles != seqs[0]->ntiles) || ((flags & SAME_NCONTIGS) && seqs[d]->ncontigs != seqs[0]->ncontigs) ||
        ((flags & SAME_LEN) && seqs[d]->len != seqs[0]->len))
      return mfx_fail(MFX_E_INVAL, "slot %u: the sequence objects of one run must hold the same contigs", d);
    if ((flags & NOT_WIDE) && evs[d]->ix->wide()) return mfx_fail(MFX_E_INVAL, "%s: k > 31 is not supported (the 128-bit kernels read one byte per base)", who);
    for (uint32_t e = 0; e < d; ++e)
      if (((flags & DISTINCT_EVALS) && evs[e] == evs[d]) || ((flags & DISTINCT_SEQS) && seqs[e] == seqs[d]))
        return mfx_fail(MFX_E_INVAL, "slots %u and %u share an evaluator or a sequence object (every slot runs on its own)", e, d);
  }
  return MFX_OK;
}

// fn(d) on a thread per slot, all at once; the first slot that failed gives the caller its code and its message
static int on_slot_threads(uint32_t ndev, const std::function<int(uint32_t)> &fn) {
  std::vector<int> rcs(ndev, MFX_OK);
  std::vector<std::string> errs(ndev);
  std::vector<std::thread> th;
  for (uint32_t d = 0; d < ndev; ++d)
    th.emplace_back([&, d] { if ((rcs[d] = fn(d)) != MFX_OK) errs[d] = mfx_last_error(); });
  for (auto &t : th) t.join();
  for (uint32_t d = 0; d < ndev; ++d)
    if (rcs[d]) return mfx_fail(rcs[d], "slot %u: %s", d, errs[d].c_str());
  return MFX_OK;
}

// The tail of a run: the result from the summed image `acc` and koverCpy, then the far K* bins that wait in the overflow list of
// every slot that ran (launched == nullptr: all), in slot order.  On failure *out is empty.
static int finish(mfx_eval *const *evs, uint32_t ndev, const uint64_t *novf, const char *launched, uint32_t nbins, const uint64_t *acc, double kover,
                  uint32_t ncontigs_total, mfx_hist_result *out) {
  int rc = mfx_hist_result_from_counts(nbins, acc, kover, ncontigs_total, out);
  for (uint32_t d = 0; d < ndev && rc == MFX_OK; ++d)
    if (!launched || launched[d]) rc = result_take_overflow(evs[d], novf[d], out);
  if (rc) mfx_hist_result_free(out);
  return rc;
}

extern "C" int mfx_hist_run_multi(mfx_eval *const *evs, const mfx_seq *const *seqs, uint32_t ndev, mfx_hist_result *out) {
  if (!evs || !seqs || !out || ndev == 0) return mfx_fail(MFX_E_INVAL, "mfx_hist_run_multi: null argument");
  int rc = check_slots("mfx_hist_run_multi", evs, seqs, ndev, SAME_NTILES | SAME_NCONTIGS | DISTINCT_EVALS);
  if (rc) return rc;
  if (ndev == 1) return mfx_hist_run(evs[0], seqs[0], out);
  const uint32_t nbins = evs[0]->nbins, ncontigs = seqs[0]->ncontigs;
  const size_t words = MFX_HIST_WORDS(nbins, ncontigs);
  // launch on every device before waiting for any; every slot works on its evaluator's own stream and image (nothing is
  // created or released per call)
  const bool timing = getenv("MFX_MULTI_TIMING") && atoi(getenv("MFX_MULTI_TIMING"));
  auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t0 = now();
  std::vector<char> launched(ndev, 0);
  for (uint32_t d = 0; d < ndev && rc == MFX_OK; ++d) {
    DevGuard g(evs[d]->device);
    rc = eval_run_enqueue(evs[d], seqs[d], d, ndev);
    launched[d] = rc == MFX_OK;
  }
  const double t1 = now();
  // the N images (~1 MB each) are added in slot order -- integers exactly, koverCpy as a fixed-order fp64 sum -- each as
  // soon as its slot is done, i.e. while the later slots still run; slot 0's pinned image is the accumulator
  uint64_t *sum = evs[0]->sr.h_img;
  double kover = 0.0, t_add = 0.0;
  std::vector<uint64_t> novf(ndev, 0);
  for (uint32_t d = 0; d < ndev; ++d) {
    if (!launched[d] && !evs[d]->sr.kern[0]) continue;
    DevGuard g(evs[d]->device);
    hipError_t e = hipStreamSynchronize(evs[d]->sr.kern[0]);
    if (e != hipSuccess && rc == MFX_OK) rc = mfx_fail(MFX_E_HIP, "mfx_hist_run_multi: slot %u failed: %s", d, hipGetErrorString(e));
    if (rc != MFX_OK) continue;
    const double ta = now();
    const uint64_t *h = evs[d]->sr.h_img;
    novf[d] = mfx_histsum::add(sum, nbins, ncontigs, h, ncontigs, nullptr);      // (slot 0: its image IS the sum)
    double kv;
    memcpy(&kv, h + words, sizeof(double));
    kover = d == 0 ? kv : kover + kv;
    t_add += now() - ta;
  }
  const double t2 = now();
  if (rc == MFX_OK) rc = finish(evs, ndev, novf.data(), nullptr, nbins, sum, kover, ncontigs, out);
  if (timing)
    fprintf(stderr, "[mfx multi] %u slots: enqueue %.3f ms, wait + add %.3f ms (of which adding the images %.3f), result %.3f ms\n", ndev, (t1 - t0) * 1e3,
            (t2 - t1) * 1e3, t_add * 1e3, (now() - t2) * 1e3);
  return rc;
}

// SURVEY 8(d)'s evaluate phase over N devices driven by one process: "first tile H2D start -> final reduced histogram on host" with the
// assembly in host memory.  Device d receives ONLY the packed planes of its share -- the tiles [T d / N, T (d + 1) / N), cut at
// multiples of 1024 tiles, plus the k - 1 bases of halo behind it -- through its own copy stream, from its own encoder threads (the
// host's threads are dealt to the slots), and evaluates the chunks as they land, exactly as the single-device run does
// (hist_run_streamed_packed).  The images are added on the host in slot order; koverCpy is bit-identical to the single launch: the
// first-level sums of the (tile, wave) values (4096 values = 1024 tiles each: the parts are cut there) are the single launch's own,
// and the host adds them in the order of mfx_sum_partials_kernel.  Contiguous shares, not the block-cyclic deal of the resident
// run: a device's share must be one stretch of the upload.  Every slot needs its own evaluator AND its own sequence object
// (mfx_seq_create on its device; they hold different parts afterwards and refuse whole-sequence calls: mfx_seq::partial).
static double sum_like_partials_kernel(const std::vector<double> &p) {
  double s[MFX_BLOCK];
  for (uint32_t t = 0; t < MFX_BLOCK; ++t) {
    double v = 0.0;
    for (size_t i = t; i < p.size(); i += MFX_BLOCK) v = v + p[i];
    s[t] = v;
  }
  for (uint32_t st = MFX_BLOCK / 2; st > 0; st >>= 1)
    for (uint32_t t = 0; t < st; ++t) s[t] = s[t] + s[t + st];
  return 0.0 + s[0];
}

static void stream_part_bounds(uint64_t T, uint32_t n, std::vector<uint64_t> &b) {
  b.assign(n + 1, 0);
  for (uint32_t d = 1; d < n; ++d) {
    uint64_t x = (uint64_t)((__uint128_t)T * d / n);
    x = (x + 512) / 1024 * 1024;
    b[d] = std::min(T, std::max(b[d - 1], x));
  }
  b[n] = T;
}

extern "C" int mfx_hist_run_streamed_multi(mfx_eval *const *evs, mfx_seq *const *seqs, uint32_t ndev, const char *const *bases, mfx_hist_result *out) {
  if (!evs || !seqs || !out || ndev == 0) return mfx_fail(MFX_E_INVAL, "mfx_hist_run_streamed_multi: null argument");
  int rc = check_slots("mfx_hist_run_streamed_multi", evs, seqs, ndev, SAME_NTILES | SAME_NCONTIGS | SAME_LEN | DISTINCT_EVALS | DISTINCT_SEQS | NOT_WIDE);
  if (rc) return rc;
  if (seqs[0]->ncontigs && !bases) return mfx_fail(MFX_E_INVAL, "mfx_hist_run_streamed_multi: null argument");
  if (ndev == 1) return mfx_hist_run_streamed(evs[0], seqs[0], bases, out);
  const uint32_t nbins = evs[0]->nbins, ncontigs = seqs[0]->ncontigs;
  std::vector<uint64_t> bound;
  stream_part_bounds(seqs[0]->ntiles, ndev, bound);
  std::vector<std::vector<double>> sums(ndev);
  const unsigned sharers = t_sharers_get() * ndev;
  rc = on_slot_threads(ndev, [&](uint32_t d) {
    mfx_host_threads_share(sharers);                          // the host's encoder threads are dealt to the slots
    StreamPart p;
    p.tl = bound[d]; p.th = bound[d + 1];
    p.chunk_sums = &sums[d];
    p.want_result = false;
    return hist_run_streamed_packed(evs[d], seqs[d], bases, nullptr, &p);
  });
  if (rc) return rc;
  uint64_t *sum = evs[0]->sr.h_img;                           // slot 0's pinned image is the accumulator
  std::vector<uint64_t> novf(ndev, 0);
  std::vector<double> all;
  for (uint32_t d = 0; d < ndev; ++d) {
    novf[d] = mfx_histsum::add(sum, nbins, ncontigs, evs[d]->sr.h_img, ncontigs, nullptr);
    all.insert(all.end(), sums[d].begin(), sums[d].end());
  }
  return finish(evs, ndev, novf.data(), nullptr, nbins, sum, sum_like_partials_kernel(all), ncontigs, out);
}

// One rank's share of the same, for the one-process-per-GPU launcher: the tiles [tile_begin, tile_end) of the assembly in host memory
// are encoded, uploaded and evaluated; counts and koverCpy are ADDED to the caller's device image (cleared by the caller; the
// launcher all-reduces it over the ranks, mfx_hist_allreduce).  Returns when the device is done.  mfx_hist_stream_share gives rank
// r of n the bounds the one-process run uses.
extern "C" int mfx_hist_run_streamed_range(mfx_eval *ev, mfx_seq *seq, const char *const *bases, uint64_t tile_begin, uint64_t tile_end,
                                           uint64_t *d_counts, double *d_kover) {
  if (!ev || !seq || !d_counts || !d_kover || (seq->ncontigs && !bases)) return mfx_fail(MFX_E_INVAL, "mfx_hist_run_streamed_range: null argument");
  if (ev->device != seq->device) return mfx_fail(MFX_E_INVAL, "evaluator and sequence live on different devices");
  if (tile_begin > tile_end || tile_end > seq->ntiles) return mfx_fail(MFX_E_INVAL, "tile range [%lu,%lu) outside [0,%lu)",
                                                                      (unsigned long)tile_begin, (unsigned long)tile_end, (unsigned long)seq->ntiles);
  if (ev->ix->wide()) return mfx_fail(MFX_E_INVAL, "mfx_hist_run_streamed_range: k > 31 is not supported");
  StreamPart p;
  p.tl = tile_begin; p.th = tile_end;
  p.d_counts = d_counts; p.d_kover = d_kover;
  p.want_result = false;
  return hist_run_streamed_packed(ev, seq, bases, nullptr, &p);
}

extern "C" int mfx_hist_stream_share(uint64_t ntiles, uint32_t rank, uint32_t nranks, uint64_t *tile_begin, uint64_t *tile_end) {
  if (!nranks || rank >= nranks || !tile_begin || !tile_end) return mfx_fail(MFX_E_INVAL, "mfx_hist_stream_share: rank %u of %u", rank, nranks);
  std::vector<uint64_t> b;
  stream_part_bounds(ntiles, nranks, b);
  *tile_begin = b[rank];
  *tile_end = b[rank + 1];
  return MFX_OK;
}

// PARTS of one assembly, one per slot, each on its own sequence-only index (mfx_index_claim_seq on the slot's contigs,
// mfx_index_count_claimed over the whole assembly, the read database update-only): every slot evaluates ITS contigs on its
// device -- no exchange of k-mers at all, whatever the size of the read database -- and the results are put together: bins and
// counters added, the per-contig counters placed at the contigs' numbers in the whole assembly (contig_ids[d][i] = number of
// slot d's contig i), koverCpy a fixed-order sum over the slots.  What config 5's -hist (15 Gb, a read database beyond one GPU)
// runs on the 8-GPU node: each device holds the slots of its contigs' k-mers only.  Slots may share a device.
extern "C" int mfx_hist_run_parts(mfx_eval *const *evs, const mfx_seq *const *seqs, const uint32_t *const *contig_ids, uint32_t ndev,
                                  uint32_t ncontigs_total, mfx_hist_result *out) {
  if (!evs || !seqs || !contig_ids || !out || ndev == 0) return mfx_fail(MFX_E_INVAL, "mfx_hist_run_parts: null argument");
  std::vector<char> seen(ncontigs_total, 0);
  int rc = check_slots("mfx_hist_run_parts", evs, seqs, ndev, DISTINCT_EVALS);
  if (rc) return rc;
  for (uint32_t d = 0; d < ndev; ++d) {
    if (seqs[d]->ncontigs && !contig_ids[d]) return mfx_fail(MFX_E_INVAL, "mfx_hist_run_parts: no contig numbers for slot %u", d);
    for (uint32_t i = 0; i < seqs[d]->ncontigs; ++i) {
      const uint32_t c = contig_ids[d][i];
      if (c >= ncontigs_total || seen[c]) return mfx_fail(MFX_E_INVAL, "slot %u: contig number %u is out of range or belongs to two slots", d, c);
      seen[c] = 1;
    }
  }
  const uint32_t nbins = evs[0]->nbins;
  std::vector<char> launched(ndev, 0);
  for (uint32_t d = 0; d < ndev && rc == MFX_OK; ++d) {
    if (seqs[d]->ntiles == 0) continue;
    DevGuard g(evs[d]->device);
    rc = eval_run_enqueue(evs[d], seqs[d], 0, 1);
    launched[d] = rc == MFX_OK;
  }
  const size_t words = MFX_HIST_WORDS(nbins, ncontigs_total);
  std::vector<uint64_t> sum(words, 0);
  double kover = 0.0;
  std::vector<uint64_t> novf(ndev, 0);
  for (uint32_t d = 0; d < ndev; ++d) {
    if (!launched[d]) continue;
    DevGuard g(evs[d]->device);
    hipError_t e = hipStreamSynchronize(evs[d]->sr.kern[0]);
    if (e != hipSuccess && rc == MFX_OK) rc = mfx_fail(MFX_E_HIP, "mfx_hist_run_parts: slot %u failed: %s", d, hipGetErrorString(e));
    if (rc != MFX_OK) continue;
    const uint32_t nc = seqs[d]->ncontigs;
    const uint64_t *h = evs[d]->sr.h_img;
    novf[d] = mfx_histsum::add(sum.data(), nbins, ncontigs_total, h, nc, contig_ids[d]);      // (launched: it has tiles, so contigs and their numbers)
    double kv;
    memcpy(&kv, h + MFX_HIST_WORDS(nbins, nc), sizeof(double));
    kover = kover + kv;                                       // slot order: a fixed-order fp64 sum
  }
  return rc ? rc : finish(evs, ndev, novf.data(), launched.data(), nbins, sum.data(), kover, ncontigs_total, out);
}

// ---------------------------------------------------------------------------
// sharded index (BASELINE config 5)
// ---------------------------------------------------------------------------
extern "C" int mfx_index_set_shard(mfx_index *ix, uint32_t rank, uint32_t nranks) {
  if (!ix || nranks == 0 || rank >= nranks || nranks > 254)
    return mfx_fail(MFX_E_INVAL, "mfx_index_set_shard: need rank < nranks <= 254");
  if (ix->seq_only && nranks > 1) return mfx_fail(MFX_E_INVAL, "a sequence-only index cannot be sharded (it is the small index: shard a full one)");
  if (ix->wide() && nranks > 1) return mfx_fail(MFX_E_INVAL, "a sharded index handles k <= 31; this index holds %d-mers", ix->k);
  DevGuard g(ix->device);
  uint64_t meta[4];
  MFX_HIP(hipMemcpy(meta, ix->d_meta, sizeof(meta), hipMemcpyDeviceToHost));
  if (meta[0] != 0) return mfx_fail(MFX_E_INVAL, "mfx_index_set_shard: the index already holds k-mers");
  ix->shard_rank = rank;
  ix->shard_n = nranks;
  return MFX_OK;
}

struct mfx_router {
  const mfx_index *ix = nullptr;
  int       device = 0;
  uint32_t  nranks = 1, max_tiles = 0;
  uint64_t *d_keys = nullptr;        // [max_tiles * TILE]
  uint8_t  *d_owner = nullptr, *d_owner2 = nullptr;
  uint32_t *d_idx = nullptr, *d_idx2 = nullptr;
  uint64_t *d_dest = nullptr;        // [256]
  void     *d_tmp = nullptr;
  size_t    tmp_bytes = 0;
  uint32_t *d_tile_cnt = nullptr;    // [max_tiles * nranks] sort-free path (nranks <= MFX_SPLIT_MAX_RANKS)
  bool      split = false;
  // buffers of the one-pass routing of mfx_hist_run_sharded, made by its first run and kept for the next ones (allocating
  // gigabytes next to tables that fill the device took up to 0.3 s of a 0.08 s run)
  struct Fused {
    uint64_t *d_keys[2] = {nullptr, nullptr}, *d_rkeys = nullptr, *d_cursors = nullptr, *h_cursors = nullptr;
    uint32_t *d_ctg[2] = {nullptr, nullptr}, *d_rctg = nullptr;
    size_t region_cap = 0, rcap = 0;
    uint32_t ndev = 0;
  } fused;
};

int mfx_sort_by_owner(void *tmp, size_t &tmp_bytes, const uint8_t *kin, uint8_t *kout, const uint32_t *vin, uint32_t *vout,
                      uint64_t n, hipStream_t st);   // mfx_sort.hip (hipcub stable radix sort)

extern "C" mfx_router *mfx_router_create(const mfx_index *ix, uint32_t nranks, uint32_t max_tiles) {
  if (ix && ix->wide()) {
    mfx_fail(MFX_E_INVAL, "mfx_router_create: a sharded index handles k <= 31; this index holds %d-mers", ix->k);
    return nullptr;
  }
  if (ix && ix->seq_only) {
    mfx_fail(MFX_E_INVAL, "mfx_router_create: a sequence-only index cannot be sharded");
    return nullptr;
  }
  if (!ix || nranks == 0 || nranks > 254 || max_tiles == 0 || (uint64_t)max_tiles * MFX_TILE >= (1ull << 31)) {
    mfx_fail(MFX_E_INVAL, "mfx_router_create: bad argument (nranks <= 254, max_tiles * %u < 2^31: the sort counts items in an int)", MFX_TILE);
    return nullptr;
  }
  DevGuard g(ix->device);
  mfx_router *r = new mfx_router;
  r->ix = ix; r->device = ix->device; r->nranks = nranks; r->max_tiles = max_tiles;
  const size_t n = (size_t)max_tiles * MFX_TILE;
  // small worlds: counting split, no position-sized scratch; MFX_ROUTE_SORT=1 forces the radix-sort path (A/B, tests)
  const char *fs = getenv("MFX_ROUTE_SORT");
  r->split = nranks <= MFX_SPLIT_MAX_RANKS && !(fs && atoi(fs));
  if (r->split) {
    if (hipMalloc((void **)&r->d_tile_cnt, (size_t)max_tiles * nranks * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc((void **)&r->d_dest, 256 * 8) != hipSuccess) {
      mfx_fail(MFX_E_NOMEM, "mfx_router_create: device allocation failed (%u tiles)", max_tiles);
      mfx_router_free(r);
      return nullptr;
    }
    return r;
  }
  size_t tb = 0;
  mfx_sort_by_owner(nullptr, tb, nullptr, nullptr, nullptr, nullptr, n, nullptr);
  r->tmp_bytes = tb;
  if (hipMalloc((void **)&r->d_keys, n * 8) != hipSuccess || hipMalloc((void **)&r->d_owner, n) != hipSuccess ||
      hipMalloc((void **)&r->d_owner2, n) != hipSuccess || hipMalloc((void **)&r->d_idx, n * 4) != hipSuccess ||
      hipMalloc((void **)&r->d_idx2, n * 4) != hipSuccess || hipMalloc((void **)&r->d_dest, 256 * 8) != hipSuccess ||
      hipMalloc(&r->d_tmp, tb ? tb : 1) != hipSuccess) {
    mfx_fail(MFX_E_NOMEM, "mfx_router_create: device allocation failed (%zu positions)", n);
    mfx_router_free(r);
    return nullptr;
  }
  return r;
}

static void router_fused_free(mfx_router *r) {
  auto &F = r->fused;
  void *p[] = {F.d_keys[0], F.d_keys[1], F.d_rkeys, F.d_cursors, F.d_ctg[0], F.d_ctg[1], F.d_rctg};
  for (void *x : p) if (x) (void)hipFree(x);
  if (F.h_cursors) (void)hipHostFree(F.h_cursors);
  F = mfx_router::Fused();
}

extern "C" void mfx_router_free(mfx_router *r) {
  if (!r) return;
  DevGuard g(r->device);
  void *p[] = {r->d_keys, r->d_owner, r->d_owner2, r->d_idx, r->d_idx2, r->d_dest, r->d_tmp, r->d_tile_cnt};
  for (void *x : p) if (x) (void)hipFree(x);
  router_fused_free(r);
  delete r;
}

// What both routers start from, the router's device being current: the shard can be routed to (canonical k-mers, odd k), the sequence
// has its bytes, and `a` asks for the tiles [tb, te), their k-mers counted into `counts`.
static int route_prepare(const mfx_router *r, const mfx_seq *seq, uint64_t tb, uint64_t te, uint32_t nbins, uint64_t *counts, mfx_route_args *a) {
  int canon = 0;
  if (int rc = index_canonical(r->ix, &canon)) return rc;
  if (!canon || !(r->ix->k & 1)) return mfx_fail(MFX_E_INVAL, "a sharded index needs a canonical k-mer database and odd k");
  if (int rc = mfx_seq_ensure_ascii(seq)) return rc;
  a->t = r->ix->view();
  a->bases = seq->d_bases;
  a->contig_off = seq->d_contig_off; a->contig_len = seq->d_contig_len; a->tile_start = seq->d_tile_start; a->tile_contig = seq->d_tile_contig;
  a->ncontigs = seq->ncontigs;
  a->tile_begin = tb; a->tile_end = te;
  a->nranks = r->nranks;
  a->keys = r->d_keys; a->owner = r->d_owner;                 // (null in a router that splits by counting)
  a->dest_counts = r->d_dest; a->tile_cnt = r->d_tile_cnt;
  a->counts = counts;
  a->nbins = nbins;
  return MFX_OK;
}

extern "C" int mfx_route_tiles(mfx_router *r, const mfx_seq *seq, uint64_t tile_begin, uint64_t tile_end, uint32_t nbins,
                               uint64_t *d_counts, uint64_t *d_keys_out, uint32_t *d_contigs_out, uint64_t *h_dest_counts,
                               void *stream) {
  if (!r || !seq || !d_counts || !d_keys_out || !d_contigs_out || !h_dest_counts)
    return mfx_fail(MFX_E_INVAL, "mfx_route_tiles: null argument");
  if (tile_begin > tile_end || tile_end > seq->ntiles || tile_end - tile_begin > r->max_tiles)
    return mfx_fail(MFX_E_INVAL, "mfx_route_tiles: tile range [%lu,%lu) invalid (max %u tiles per call)",
                    (unsigned long)tile_begin, (unsigned long)tile_end, r->max_tiles);
  DevGuard g(r->device);
  hipStream_t st = (hipStream_t)stream;
  const uint64_t n = (tile_end - tile_begin) * MFX_TILE;
  mfx_route_args a;
  int rc = route_prepare(r, seq, tile_begin, tile_end, nbins, d_counts, &a);
  if (rc) return rc;
  if (r->split) {
    MFX_HIP(mfx_k_route_split(a, d_keys_out, d_contigs_out, st));
    for (uint32_t i = 0; i < r->nranks; ++i) h_dest_counts[i] = 0;
    if (tile_end > tile_begin) {
      MFX_HIP(hipMemcpyAsync(h_dest_counts, r->d_dest, r->nranks * 8, hipMemcpyDeviceToHost, st));
      MFX_HIP(hipStreamSynchronize(st));
    }
    return MFX_OK;
  }
  MFX_HIP(hipMemsetAsync(r->d_dest, 0, 256 * 8, st));
  MFX_HIP(mfx_k_route(a, st));
  MFX_HIP(mfx_k_iota(r->d_idx, n, st));
  // stable sort by owner: within a destination the k-mers keep their sequence order,
  // so the owner's fp64 koverCpy sum is reproducible
  rc = mfx_sort_by_owner(r->d_tmp, r->tmp_bytes, r->d_owner, r->d_owner2, r->d_idx, r->d_idx2, n, st);
  if (rc) return rc;
  MFX_HIP(hipMemcpyAsync(h_dest_counts, r->d_dest, r->nranks * 8, hipMemcpyDeviceToHost, st));
  MFX_HIP(hipStreamSynchronize(st));
  uint64_t nvalid = 0;
  for (uint32_t i = 0; i < r->nranks; ++i) nvalid += h_dest_counts[i];
  MFX_HIP(mfx_k_route_gather(a, r->d_idx2, nvalid, d_keys_out, d_contigs_out, st));
  // the groups are complete when this returns, as on the split path: callers hand them to OTHER streams right away
  // (mfx_hist_run_sharded: the owners' peer copies), which nothing else orders behind this gather
  MFX_HIP(hipStreamSynchronize(st));
  return MFX_OK;
}

// the owner side's launch arguments but for the k-mers themselves
static mfx_hist_keys_args keys_args(const mfx_eval *ev, uint32_t ncontigs, uint64_t *d_counts) {
  mfx_hist_keys_args a;
  a.t = ev->ix->view();
  a.ks.peak = ev->peak; a.ks.n_prob = ev->n_prob; a.ks.probK = ev->d_probK; a.ks.probP = ev->d_probP;
  a.ks.nbins = ev->nbins; a.ks.ncontigs = ncontigs; a.ks.counts = d_counts;
  a.ks.partials = ev->d_partials; a.ks.ovf = ev->d_ovf;
  return a;
}

extern "C" int mfx_hist_keys_launch(mfx_eval *ev, const uint64_t *d_keys, const uint32_t *d_contigs, uint64_t n,
                                    uint32_t ncontigs, uint64_t *d_counts, double *d_kover, void *stream) {
  if (!ev || !d_counts || !d_kover || (n && (!d_keys || !d_contigs))) return mfx_fail(MFX_E_INVAL, "mfx_hist_keys_launch: null argument");
  if (ev->ix->wide()) return mfx_fail(MFX_E_INVAL, "mfx_hist_keys_launch: a sharded index handles k <= 31");
  if (ev->ix->seq_only) return mfx_fail(MFX_E_INVAL, "mfx_hist_keys_launch: a sequence-only index holds the k-mers of one sequence, the sharded path needs a full (sharded) one; build a full index (mfx_index_create)");
  DevGuard g(ev->device);
  mfx_hist_keys_args a = keys_args(ev, ncontigs, d_counts);
  a.keys = d_keys;
  a.contig = d_contigs;
  a.n = n;
  MFX_HIP(mfx_k_hist_keys(a, ev->grid, (hipStream_t)stream));
  MFX_HIP(mfx_k_sum_partials(ev->d_partials, (uint32_t)ev->grid, d_kover, (hipStream_t)stream));
  return MFX_OK;
}

// The slots of a sharded run: slot d holds shard d of ndev, its router is built on that shard for ndev ranks, and all slots see the same
// sequence and route the same number of tiles per round.
static int check_shards(mfx_eval *const *evs, mfx_router *const *routers, const mfx_seq *const *seqs, uint32_t ndev, mfx_hist_result *out) {
  if (!evs || !routers || !seqs || !out || ndev == 0) return mfx_fail(MFX_E_INVAL, "mfx_hist_run_sharded: null argument");
  if (int rc = check_slots("mfx_hist_run_sharded", evs, seqs, ndev, SAME_NTILES | SAME_NCONTIGS)) return rc;
  for (uint32_t d = 0; d < ndev; ++d) {
    const mfx_index *ix = evs[d]->ix;
    if (!routers[d] || ix->shard_n != ndev || ix->shard_rank != d || routers[d]->ix != ix || routers[d]->nranks != ndev)
      return mfx_fail(MFX_E_INVAL, "slot %u: its index must be shard %u of %u (mfx_index_set_shard) and its router built on it for %u ranks", d, d, ndev, ndev);
    if (routers[d]->max_tiles != routers[0]->max_tiles) return mfx_fail(MFX_E_INVAL, "slot %u: the routers of one run must route the same number of tiles per round", d);
  }
  return MFX_OK;
}

// every slot's device may read every other slot's (the owners take their groups where the sources wrote them)
static void enable_peer_access(mfx_eval *const *evs, uint32_t ndev) {
  for (uint32_t d = 0; d < ndev; ++d)
    for (uint32_t e = 0; e < ndev; ++e) {
      if (evs[e]->device == evs[d]->device) continue;
      DevGuard g(evs[d]->device);
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, evs[d]->device, evs[e]->device) == hipSuccess && can && hipDeviceEnablePeerAccess(evs[e]->device, 0) != hipSuccess)
        (void)hipGetLastError();                              // already enabled
    }
}

namespace {
struct Stream {   // a stream of a run: waited for and destroyed on scope exit
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream &) = delete;                            // (one owner: the destructor destroys the stream)
  hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
  operator hipStream_t() const { return s; }
  ~Stream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
};

// The per-slot state of a sharded run is released on every way out of the run, slot by slot with the slot's device current.  A Slot
// declares its streams BEHIND its buffers: they are waited for and destroyed before the buffers are freed.
template <class Slot>
struct SlotsRelease {
  std::vector<Slot> &sl;
  ~SlotsRelease() { while (!sl.empty()) { DevGuard g(sl.back().device); sl.pop_back(); } }
};
}  // namespace

// Sharded index driven by ONE process (BASELINE config 5 from the C++ side): slot d holds shard d of N of the
// k-mer table on its own device.  Per round, every slot routes a chunk of ITS tile range (k-mers grouped by owner,
// sequence order kept), the groups travel to their owners by peer copy over xGMI -- the all-to-all of the
// one-process-per-GPU form (merfin_amd/distributed.py::sharded_hist) -- and every owner probes / computes K* / bins
// what it received, source by source in slot order (so koverCpy is a fixed-order sum).  The N counts images are added
// on the host; kasm was counted at the sources, kmissing / bins / koverCpy at the owners.
static int hist_run_sharded_ordered(mfx_eval *const *evs, mfx_router *const *routers, const mfx_seq *const *seqs, uint32_t ndev,
                                    mfx_hist_result *out) {
  const uint32_t nbins = evs[0]->nbins, ncontigs = seqs[0]->ncontigs, per = routers[0]->max_tiles;
  const uint64_t T = seqs[0]->ntiles;
  const size_t words = MFX_HIST_WORDS(nbins, ncontigs), cap = (size_t)per * MFX_TILE;
  const size_t rcap = cap + cap / 2 + 4096;                  // receive side: a balanced owner gets ~cap k-mers per round
  struct Slot {
    int device = 0;
    DevBuf<uint64_t> d_counts, d_keys, d_rkeys;
    DevBuf<uint32_t> d_ctg, d_rctg;
    DevBuf<double> d_kover;
    Stream st;
    std::vector<uint64_t> dest;      // k-mers this slot routed to each owner in the current round
  };
  std::vector<Slot> sl(ndev);
  SlotsRelease<Slot> on_exit{sl};
  int rc = MFX_OK;
  for (uint32_t d = 0; d < ndev && rc == MFX_OK; ++d) {
    DevGuard g(evs[d]->device);
    Slot &S = sl[d];
    S.device = evs[d]->device;
    S.dest.assign(ndev, 0);
    if (S.st.create() != hipSuccess || S.d_counts.alloc(words) != hipSuccess || S.d_kover.alloc(1) != hipSuccess ||
        S.d_keys.alloc(cap) != hipSuccess || S.d_rkeys.alloc(rcap) != hipSuccess || S.d_ctg.alloc(cap) != hipSuccess || S.d_rctg.alloc(rcap) != hipSuccess ||
        hipMemsetAsync(S.d_counts.p, 0, words * sizeof(uint64_t), S.st) != hipSuccess || hipMemsetAsync(S.d_kover.p, 0, sizeof(double), S.st) != hipSuccess ||
        mfx_ovf_reset_async(evs[d], S.st) != MFX_OK)
      rc = mfx_fail(MFX_E_NOMEM, "mfx_hist_run_sharded: buffers for slot %u (%zu k-mers per round) could not be set up", d, cap);
  }
  const uint64_t rounds = ((T + ndev - 1) / ndev + per - 1) / per;
  for (uint64_t r = 0; r < rounds && rc == MFX_OK; ++r) {
    // ---- route: all slots at once (each call blocks until its group sizes are on the host)
    rc = on_slot_threads(ndev, [&](uint32_t d) {
      const uint64_t lo = T * d / ndev, hi = T * (d + 1) / ndev;
      const uint64_t tb = std::min(hi, lo + r * per), te = std::min(hi, tb + per);
      return mfx_route_tiles(routers[d], seqs[d], tb, te, nbins, sl[d].d_counts.p, sl[d].d_keys.p, sl[d].d_ctg.p, sl[d].dest.data(), sl[d].st);
    });
    if (rc) break;
    // ---- exchange + evaluate: owner o takes its group from every source in slot order
    for (uint32_t o = 0; o < ndev && rc == MFX_OK; ++o) {
      DevGuard g(evs[o]->device);
      // the groups of all sources land one behind the other (slot order) and are evaluated by ONE launch: a launch per
      // source was 8x the launches, each with its own ramp-up and tail.  (Should the owners be so unbalanced that one
      // owner's share of a round outgrows its buffer, it takes its groups source by source.)
      uint64_t total = 0;
      for (uint32_t s2 = 0; s2 < ndev; ++s2) total += sl[s2].dest[o];
      const bool merged = total <= rcap;
      uint64_t at = 0;
      for (uint32_t s2 = 0; s2 < ndev && rc == MFX_OK; ++s2) {
        const uint64_t n = sl[s2].dest[o];
        if (!n) continue;
        uint64_t off = 0;
        for (uint32_t q = 0; q < o; ++q) off += sl[s2].dest[q];
        hipError_t e = hipMemcpyPeerAsync(sl[o].d_rkeys.p + at, evs[o]->device, sl[s2].d_keys.p + off, evs[s2]->device, n * 8, sl[o].st);
        if (e == hipSuccess) e = hipMemcpyPeerAsync(sl[o].d_rctg.p + at, evs[o]->device, sl[s2].d_ctg.p + off, evs[s2]->device, n * 4, sl[o].st);
        if (e != hipSuccess) { rc = mfx_fail(MFX_E_HIP, "peer copy of %lu routed k-mers from slot %u to slot %u failed: %s", (unsigned long)n, s2, o, hipGetErrorString(e)); break; }
        if (merged) at += n;
        else rc = mfx_hist_keys_launch(evs[o], sl[o].d_rkeys.p, sl[o].d_rctg.p, n, ncontigs, sl[o].d_counts.p, sl[o].d_kover.p, sl[o].st);
      }
      if (merged && at && rc == MFX_OK)
        rc = mfx_hist_keys_launch(evs[o], sl[o].d_rkeys.p, sl[o].d_rctg.p, at, ncontigs, sl[o].d_counts.p, sl[o].d_kover.p, sl[o].st);
    }
    // the sources' buffers are rewritten by the next round's routing: every owner must have taken its groups
    for (uint32_t d = 0; d < ndev; ++d) {
      DevGuard g(evs[d]->device);
      if (hipStreamSynchronize(sl[d].st) != hipSuccess && rc == MFX_OK) rc = mfx_fail(MFX_E_HIP, "mfx_hist_run_sharded: slot %u failed: %s", d, hipGetErrorString(hipGetLastError()));
    }
  }
  std::vector<uint64_t> sum(words, 0), h(words), novf(ndev, 0);
  double kover = 0.0;
  for (uint32_t d = 0; d < ndev && rc == MFX_OK; ++d) {
    DevGuard g(evs[d]->device);
    double kv = 0.0;
    if (hipMemcpy(h.data(), sl[d].d_counts.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&kv, sl[d].d_kover.p, sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) { rc = mfx_fail(MFX_E_HIP, "mfx_hist_run_sharded: D2H of slot %u failed", d); break; }
    novf[d] = mfx_histsum::add(sum.data(), nbins, ncontigs, h.data(), ncontigs, nullptr);
    kover = kover + kv;                                       // slot order: fixed-order fp64 sum
  }
  return rc ? rc : finish(evs, ndev, novf.data(), nullptr, nbins, sum.data(), kover, ncontigs, out);
}


// The same run with the ONE-PASS router (mfx_route_fused_kernel) and owners that evaluate the groups WHERE THEY LIE
// (mfx_hist_keys_kernel<true>: up to 16 segments per launch): a tile is decoded once instead of twice, no per-tile prefix, a
// group whose source shares the owner's device is not copied at all, and the routing of round r + 1 runs under the owners'
// evaluation of round r (two sets of group buffers).  The price is the ORDER of an owner's k-mers, which only the fp64 sum of
// koverCpy ever needed: the owners sum it in fixed point (units of 2^-52, 128-bit integers -- adds commute), so the result is
// still bit-identical run to run, whatever the devices and the scheduling.  Taken when every slot is one of <= 16 ranks and
// every prob of the K* table lies in [0, 4096) (the fixed-point range); else hist_run_sharded_ordered.  A round so unbalanced
// that an owner's region overflows (a megabase of one repeated minimizer) is routed again by the exact counting split.
extern "C" int mfx_hist_run_sharded(mfx_eval *const *evs, mfx_router *const *routers, const mfx_seq *const *seqs, uint32_t ndev,
                                    mfx_hist_result *out) {
  if (int crc = check_shards(evs, routers, seqs, ndev, out)) return crc;
  enable_peer_access(evs, ndev);
  bool fused = ndev <= MFX_KEYS_MAX_SEGS && ndev <= MFX_SPLIT_MAX_RANKS;
  for (uint32_t d = 0; d < ndev && fused; ++d) {
    if (!routers[d]->split || evs[d]->ix->wide() || evs[d]->ix->seq_only) fused = false;
    for (double p : evs[d]->probP) if (!(p >= 0.0 && p < 4096.0)) fused = false;
  }
  if (const char *e = getenv("MFX_SHARDED_ORDERED")) if (atoi(e)) fused = false;      // A/B, tests: the ordered form
  if (!fused) return hist_run_sharded_ordered(evs, routers, seqs, ndev, out);

  const uint32_t nbins = evs[0]->nbins, ncontigs = seqs[0]->ncontigs, per = routers[0]->max_tiles;
  const uint64_t T = seqs[0]->ntiles;
  const size_t words = MFX_HIST_WORDS(nbins, ncontigs), cap = (size_t)per * MFX_TILE;
  const size_t region_cap = cap / ndev + cap / (4 * ndev) + 2 * MFX_TILE;     // an owner's share of a round: 1/N of it + 25 % + two tiles
  bool any_remote = false;
  for (uint32_t d = 1; d < ndev; ++d) if (evs[d]->device != evs[0]->device) any_remote = true;
  const size_t rcap = any_remote ? cap + cap / 2 + 4096 : 0;                 // receive side of the groups that come from other devices
  struct Slot {
    int device = 0;
    DevBuf<uint64_t> d_counts, d_kfix, d_pkeys;
    DevBuf<uint32_t> d_pctg;
    DevBuf<double> d_kover;                                      // (the exact fallback's ordered partial sums land here)
    Stream rst, ost;                                             // (the group buffers are the router's: mfx_router::Fused)
    // the groups this slot routed in a round: [set][owner] -> where and how many
    std::vector<const uint64_t *> gkeys[2];
    std::vector<const uint32_t *> gctg[2];
    std::vector<uint64_t> gn[2];
  };
  std::vector<Slot> sl(ndev);
  SlotsRelease<Slot> on_exit{sl};
  int rc = MFX_OK;
  for (uint32_t d = 0; d < ndev && rc == MFX_OK; ++d) {
    DevGuard g(evs[d]->device);
    Slot &S = sl[d];
    S.device = evs[d]->device;
    for (int b2 = 0; b2 < 2; ++b2) { S.gkeys[b2].assign(ndev, nullptr); S.gctg[b2].assign(ndev, nullptr); S.gn[b2].assign(ndev, 0); }
    bool ok = S.rst.create() == hipSuccess && S.ost.create() == hipSuccess &&
              S.d_counts.alloc(words) == hipSuccess && S.d_kover.alloc(1) == hipSuccess && S.d_kfix.alloc(2) == hipSuccess;
    // the group buffers live in the router (made by the first run on it)
    auto &F = routers[d]->fused;
    if (ok && (F.region_cap != region_cap || F.rcap != rcap || F.ndev != ndev)) {
      router_fused_free(routers[d]);
      F.region_cap = region_cap; F.rcap = rcap; F.ndev = ndev;
      ok = hipMalloc((void **)&F.d_cursors, 2 * (ndev + 1) * sizeof(uint64_t)) == hipSuccess &&
           hipHostMalloc((void **)&F.h_cursors, 2 * (ndev + 1) * sizeof(uint64_t), hipHostMallocDefault) == hipSuccess;
      for (int b2 = 0; b2 < 2 && ok; ++b2)
        ok = hipMalloc((void **)&F.d_keys[b2], (size_t)ndev * region_cap * 8) == hipSuccess && hipMalloc((void **)&F.d_ctg[b2], (size_t)ndev * region_cap * 4) == hipSuccess;
      if (ok && rcap) ok = hipMalloc((void **)&F.d_rkeys, rcap * 8) == hipSuccess && hipMalloc((void **)&F.d_rctg, rcap * 4) == hipSuccess;
      if (!ok) router_fused_free(routers[d]);
    }
    ok = ok && hipMemsetAsync(S.d_counts.p, 0, words * sizeof(uint64_t), S.ost) == hipSuccess && hipMemsetAsync(S.d_kover.p, 0, sizeof(double), S.ost) == hipSuccess &&
         hipMemsetAsync(S.d_kfix.p, 0, 2 * sizeof(uint64_t), S.ost) == hipSuccess && mfx_ovf_reset_async(evs[d], S.ost) == MFX_OK &&
         hipStreamSynchronize(S.ost) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); rc = mfx_fail(MFX_E_NOMEM, "mfx_hist_run_sharded: buffers for slot %u (%zu k-mers per round) could not be set up", d, cap); }
  }
  const uint64_t rounds = ((T + ndev - 1) / ndev + per - 1) / per;
  // ---- route round r of every slot into buffer set b2 (one host thread per slot; returns when the group sizes are on the host)
  auto route_round = [&](uint64_t r, int b2) {
    return on_slot_threads(ndev, [&, r, b2](uint32_t d) -> int {
      Slot &S = sl[d];
      const uint64_t lo = T * d / ndev, hi = T * (d + 1) / ndev;
      const uint64_t tb = std::min(hi, lo + r * per), te = std::min(hi, tb + per);
      for (uint32_t o = 0; o < ndev; ++o) { S.gn[b2][o] = 0; S.gkeys[b2][o] = nullptr; S.gctg[b2][o] = nullptr; }
      if (te <= tb) return MFX_OK;
      DevGuard g(evs[d]->device);
      const auto &F = routers[d]->fused;
      auto fail = [](int code, const char *what, hipError_t e) { (void)hipGetLastError(); return mfx_fail(code, "%s: %s", what, hipGetErrorString(e)); };
      mfx_route_args a;
      if (int erc = route_prepare(routers[d], seqs[d], tb, te, nbins, S.d_counts.p, &a)) return erc;
      uint64_t *cur = F.d_cursors + (size_t)b2 * (ndev + 1), *hcur = F.h_cursors + (size_t)b2 * (ndev + 1);      // h_cursors: pinned, [2][ndev + 1]
      hipError_t e = hipMemsetAsync(cur, 0, (ndev + 1) * sizeof(uint64_t), S.rst);
      if (e == hipSuccess) e = mfx_k_route_fused(a, F.d_keys[b2], F.d_ctg[b2], cur, region_cap, S.rst);
      if (e == hipSuccess) e = hipMemcpyAsync(hcur, cur, (ndev + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, S.rst);
      if (e == hipSuccess) e = hipStreamSynchronize(S.rst);
      if (e != hipSuccess) return fail(MFX_E_HIP, "routing failed", e);
      if (hcur[ndev] == 0) {
        for (uint32_t o = 0; o < ndev; ++o) { S.gn[b2][o] = hcur[o]; S.gkeys[b2][o] = F.d_keys[b2] + (size_t)o * region_cap; S.gctg[b2][o] = F.d_ctg[b2] + (size_t)o * region_cap; }
        return MFX_OK;
      }
      // an owner's region overflowed: this round of this slot again, by the exact counting split into a packed buffer.  (The one-pass
      // kernel counted the round's k-mers into kasm already: the split's own count is taken back out below.)
      if (!S.d_pkeys.p) {
        e = S.d_pkeys.alloc(2 * cap);
        if (e == hipSuccess) e = S.d_pctg.alloc(2 * cap);
        if (e != hipSuccess) return fail(MFX_E_NOMEM, "no memory for the exact re-routing of an unbalanced round", e);
      }
      // kasm (global + per contig) would be counted twice: the exact split counts into a scratch image instead
      DevBuf<uint64_t> scratch;
      e = scratch.alloc(words);
      if (e == hipSuccess) e = hipMemsetAsync(scratch.p, 0, words * sizeof(uint64_t), S.rst);
      a.counts = scratch.p;
      uint64_t *pk = S.d_pkeys.p + (size_t)b2 * cap;
      uint32_t *pc = S.d_pctg.p + (size_t)b2 * cap;
      if (e == hipSuccess) e = mfx_k_route_split(a, pk, pc, S.rst);
      uint64_t hd[MFX_SPLIT_MAX_RANKS] = {0};
      if (e == hipSuccess) e = hipMemcpyAsync(hd, routers[d]->d_dest, ndev * 8, hipMemcpyDeviceToHost, S.rst);
      if (e == hipSuccess) e = hipStreamSynchronize(S.rst);
      if (e != hipSuccess) return fail(MFX_E_HIP, "exact re-routing failed", e);
      uint64_t at = 0;
      for (uint32_t o = 0; o < ndev; ++o) { S.gn[b2][o] = hd[o]; S.gkeys[b2][o] = pk + at; S.gctg[b2][o] = pc + at; at += hd[o]; }
      return MFX_OK;
    });
  };
  if (rounds && rc == MFX_OK) rc = route_round(0, 0);
  for (uint64_t r = 0; r < rounds && rc == MFX_OK; ++r) {
    const int b2 = (int)(r & 1);
    // ---- owners: one launch over the groups of all sources; a group on another device travels by peer copy first
    for (uint32_t o = 0; o < ndev && rc == MFX_OK; ++o) {
      DevGuard g(evs[o]->device);
      Slot &O = sl[o];
      const auto &F = routers[o]->fused;
      mfx_hist_keys_args a = keys_args(evs[o], ncontigs, O.d_counts.p);
      a.kfix = O.d_kfix.p;
      uint64_t at = 0, total = 0;
      for (uint32_t s2 = 0; s2 < ndev && rc == MFX_OK; ++s2) {
        const uint64_t n = sl[s2].gn[b2][o];
        if (!n) continue;
        const uint64_t *kp = sl[s2].gkeys[b2][o];
        const uint32_t *cp = sl[s2].gctg[b2][o];
        if (evs[s2]->device != evs[o]->device) {
          if (at + n > rcap) { rc = mfx_fail(MFX_E_FULL, "mfx_hist_run_sharded: owner %u receives more than %zu k-mers in one round", o, rcap); break; }
          hipError_t e = hipMemcpyPeerAsync(F.d_rkeys + at, evs[o]->device, kp, evs[s2]->device, n * 8, O.ost);
          if (e == hipSuccess) e = hipMemcpyPeerAsync(F.d_rctg + at, evs[o]->device, cp, evs[s2]->device, n * 4, O.ost);
          if (e != hipSuccess) { rc = mfx_fail(MFX_E_HIP, "peer copy of %lu routed k-mers from slot %u to slot %u failed: %s", (unsigned long)n, s2, o, hipGetErrorString(e)); break; }
          kp = F.d_rkeys + at; cp = F.d_rctg + at;
          at += n;
        }
        a.seg_keys[a.nseg] = kp; a.seg_contig[a.nseg] = cp; a.seg_n[a.nseg] = n;
        ++a.nseg;
        total += n;
      }
      a.n = total;
      if (rc == MFX_OK && total) {
        hipError_t e = mfx_k_hist_keys(a, evs[o]->grid, O.ost);
        if (e != hipSuccess) rc = mfx_fail(MFX_E_HIP, "mfx_hist_run_sharded: owner launch of slot %u failed: %s", o, hipGetErrorString(e));
      }
    }
    // ---- the next round is routed (into the other buffer set) while the owners evaluate this one
    if (r + 1 < rounds && rc == MFX_OK) rc = route_round(r + 1, b2 ^ 1);
    // this round's groups are consumed before the round after the next overwrites their buffers
    for (uint32_t d = 0; d < ndev; ++d) {
      DevGuard g(evs[d]->device);
      if (hipStreamSynchronize(sl[d].ost) != hipSuccess && rc == MFX_OK) rc = mfx_fail(MFX_E_HIP, "mfx_hist_run_sharded: slot %u failed: %s", d, hipGetErrorString(hipGetLastError()));
    }
  }
  std::vector<uint64_t> sum(words, 0), h(words), novf(ndev, 0);
  unsigned __int128 kfix = 0;
  for (uint32_t d = 0; d < ndev && rc == MFX_OK; ++d) {
    DevGuard g(evs[d]->device);
    uint64_t kf[2] = {0, 0};
    if (hipMemcpy(h.data(), sl[d].d_counts.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(kf, sl[d].d_kfix.p, sizeof(kf), hipMemcpyDeviceToHost) != hipSuccess) { rc = mfx_fail(MFX_E_HIP, "mfx_hist_run_sharded: D2H of slot %u failed", d); break; }
    novf[d] = mfx_histsum::add(sum.data(), nbins, ncontigs, h.data(), ncontigs, nullptr);
    kfix += ((unsigned __int128)kf[1] << 64) | kf[0];           // integers: the order of the slots does not matter either
  }
  // koverCpy = kfix * 2^-52 (the same three roundings whatever the run: deterministic)
  const double kover = ((double)(uint64_t)(kfix >> 64) * 18446744073709551616.0 + (double)(uint64_t)kfix) / 4503599627370496.0;
  return rc ? rc : finish(evs, ndev, novf.data(), nullptr, nbins, sum.data(), kover, ncontigs, out);
}

