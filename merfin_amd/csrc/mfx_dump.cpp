// mfx_dump.cpp -- -dump: the per-position values of a contig (one evaluator or an index sharded over several), the host-thread
// budget of the text formatting, and the writer of the dump text.
#include "mfx_host.h"
#include "mfx_kernels.h"
#include "mfx_pipe.h"

#include <fcntl.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

// ---------------------------------------------------------------------------
// -dump
// ---------------------------------------------------------------------------
extern "C" int mfx_dump_values(mfx_eval *ev, const mfx_seq *seq, uint32_t contig, uint64_t pos_begin, uint64_t pos_end,
                               uint32_t *readV, uint32_t *asmV, uint64_t *kasm, uint64_t *kmissing) {
  if (!ev || !seq || !readV || !asmV) return mfx_fail(MFX_E_INVAL, "mfx_dump_values: null argument");
  if (contig >= seq->ncontigs || pos_begin > pos_end || pos_end > seq->len[contig])
    return mfx_fail(MFX_E_INVAL, "mfx_dump_values: range [%lu,%lu) outside contig %u of length %lu",
                    (unsigned long)pos_begin, (unsigned long)pos_end, contig,
                    (unsigned long)(contig < seq->ncontigs ? seq->len[contig] : 0));
  if (int erc = mfx_seq_ensure_ascii(seq)) return erc;
  DevGuard g(ev->device);
  int canon = 0;
  int rc = index_canonical(ev->ix, &canon);
  if (rc) return rc;
  if ((rc = mfx_check_seq_of_index(ev->ix, seq, "-dump")) != MFX_OK) return rc;
  uint64_t n = pos_end - pos_begin;
  if (kasm) *kasm = 0;
  if (kmissing) *kmissing = 0;
  if (n == 0) return MFX_OK;
  uint64_t tb = pos_begin / MFX_TILE * MFX_TILE;     // tile-aligned start keeps the 16-byte loads aligned
  DevBuf<uint32_t> dr, da;
  DevBuf<uint64_t> ds;
  MFX_HIP(dr.alloc(n));
  MFX_HIP(da.alloc(n));
  MFX_HIP(ds.alloc(2));
  MFX_HIP(mfx_memset_now(ds.p, 0, 2 * sizeof(uint64_t)));
  const mfx_dump_args a = dump_args_of(ev, canon, seq->d_bases + seq->off[contig] + tb, pos_end - tb, pos_begin - tb, seq->len[contig] - tb, dr.p, da.p, ds.p);
  MFX_HIP(ev->ix->wide() ? mfx_kw_dump(a, nullptr) : mfx_k_dump(a, nullptr));
  MFX_HIP(hipMemcpy(readV, dr.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  MFX_HIP(hipMemcpy(asmV, da.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  uint64_t st[2];
  MFX_HIP(hipMemcpy(st, ds.p, sizeof(st), hipMemcpyDeviceToHost));
  if (kasm) *kasm = st[0];
  if (kmissing) *kmissing = st[1];
  return MFX_OK;
}

// The same values over an index SHARDED across N evaluators (mfx_index_set_shard): every k-mer has one owner and the
// other shards answer 0, so each slot runs the lookup kernel over its copy of the sequence against its own shard and
// the N value arrays are ADDED on slot 0's device (peer copies, 8 B per position and slot).  kmissing is then
// counted from the summed values (readK == 0 is not additive over shards).
extern "C" int mfx_dump_values_sharded(mfx_eval *const *evs, const mfx_seq *const *seqs, uint32_t nslots, uint32_t contig,
                                       uint64_t pos_begin, uint64_t pos_end, uint32_t *readV, uint32_t *asmV,
                                       uint64_t *kasm, uint64_t *kmissing) {
  if (!evs || !seqs || nslots == 0 || !readV || !asmV) return mfx_fail(MFX_E_INVAL, "mfx_dump_values_sharded: null argument");
  for (uint32_t d = 0; d < nslots; ++d) {
    if (!evs[d] || !seqs[d]) return mfx_fail(MFX_E_INVAL, "mfx_dump_values_sharded: slot %u is null", d);
    const mfx_index *ix = evs[d]->ix;
    if (ix->shard_n != nslots || ix->shard_rank != d)
      return mfx_fail(MFX_E_INVAL, "slot %u: its index must be shard %u of %u (mfx_index_set_shard)", d, d, nslots);
    if (ix->wide()) return mfx_fail(MFX_E_INVAL, "a sharded index handles k <= 31");
    if (evs[d]->device != seqs[d]->device || seqs[d]->ncontigs != seqs[0]->ncontigs || contig >= seqs[d]->ncontigs ||
        seqs[d]->len[contig] != seqs[0]->len[contig])
      return mfx_fail(MFX_E_INVAL, "slot %u: the sequences must be copies of one another, each on its evaluator's device", d);
    if (int erc = mfx_seq_ensure_ascii(seqs[d])) return erc;
  }
  const mfx_seq *seq0 = seqs[0];
  if (pos_begin > pos_end || pos_end > seq0->len[contig])
    return mfx_fail(MFX_E_INVAL, "mfx_dump_values_sharded: range [%lu,%lu) outside contig %u of length %lu",
                    (unsigned long)pos_begin, (unsigned long)pos_end, contig, (unsigned long)seq0->len[contig]);
  const uint64_t n = pos_end - pos_begin;
  if (kasm) *kasm = 0;
  if (kmissing) *kmissing = 0;
  if (n == 0) return MFX_OK;
  const uint64_t tb = pos_begin / MFX_TILE * MFX_TILE;
  struct Slot { uint32_t *dr = nullptr, *da = nullptr; uint64_t *ds = nullptr; };
  std::vector<Slot> sl(nslots);
  uint32_t *tr = nullptr, *ta = nullptr;                       // slot 0's landing buffers for a peer's arrays
  auto release = [&]() {
    for (uint32_t d = 0; d < nslots; ++d) {
      DevGuard g(evs[d]->device);
      if (sl[d].dr) (void)hipFree(sl[d].dr);
      if (sl[d].da) (void)hipFree(sl[d].da);
      if (sl[d].ds) (void)hipFree(sl[d].ds);
    }
    DevGuard g(evs[0]->device);
    if (tr) (void)hipFree(tr);
    if (ta) (void)hipFree(ta);
  };
  auto args_of = [&](uint32_t d, int canon) {
    return dump_args_of(evs[d], canon, seqs[d]->d_bases + seqs[d]->off[contig] + tb, pos_end - tb, pos_begin - tb, seqs[d]->len[contig] - tb, sl[d].dr, sl[d].da, sl[d].ds);
  };
  int rc = MFX_OK;
  hipError_t e = hipSuccess;
  for (uint32_t d = 0; d < nslots && rc == MFX_OK && e == hipSuccess; ++d) {          // every shard's lookup, all devices at once
    DevGuard g(evs[d]->device);
    int canon = 0;
    rc = index_canonical(evs[d]->ix, &canon);
    if (rc) break;
    e = hipMalloc((void **)&sl[d].dr, n * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&sl[d].da, n * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&sl[d].ds, 2 * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMemsetAsync(sl[d].ds, 0, 2 * sizeof(uint64_t), nullptr);
    if (e != hipSuccess) break;
    e = mfx_k_dump(args_of(d, canon), nullptr);
  }
  for (uint32_t d = 0; d < nslots && rc == MFX_OK && e == hipSuccess; ++d) {
    DevGuard g(evs[d]->device);
    e = hipDeviceSynchronize();
  }
  if (rc == MFX_OK && e == hipSuccess && nslots > 1) {
    DevGuard g(evs[0]->device);
    e = hipMalloc((void **)&tr, n * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&ta, n * sizeof(uint32_t));
    for (uint32_t d = 1; d < nslots && e == hipSuccess; ++d) {
      if (evs[d]->device == evs[0]->device) {
        e = mfx_k_add_u32(sl[0].dr, sl[d].dr, n, nullptr);
        if (e == hipSuccess) e = mfx_k_add_u32(sl[0].da, sl[d].da, n, nullptr);
        continue;
      }
      e = hipMemcpyPeerAsync(tr, evs[0]->device, sl[d].dr, evs[d]->device, n * sizeof(uint32_t), nullptr);
      if (e == hipSuccess) e = hipMemcpyPeerAsync(ta, evs[0]->device, sl[d].da, evs[d]->device, n * sizeof(uint32_t), nullptr);
      if (e == hipSuccess) e = mfx_k_add_u32(sl[0].dr, tr, n, nullptr);
      if (e == hipSuccess) e = mfx_k_add_u32(sl[0].da, ta, n, nullptr);
    }
    if (e == hipSuccess) e = hipMemsetAsync(sl[0].ds, 0, 2 * sizeof(uint64_t), nullptr);
    if (e == hipSuccess) {
      mfx_dump_args a = args_of(0, 0);
      a.recount = 1;
      e = mfx_k_dump(a, nullptr);
    }
  }
  if (rc == MFX_OK && e == hipSuccess) {
    DevGuard g(evs[0]->device);
    uint64_t st[2] = {0, 0};
    e = hipMemcpy(readV, sl[0].dr, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(asmV, sl[0].da, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(st, sl[0].ds, sizeof(st), hipMemcpyDeviceToHost);
    if (kasm) *kasm = st[0];
    if (kmissing) *kmissing = st[1];
  }
  release();
  if (rc == MFX_OK && e != hipSuccess) rc = mfx_fail(MFX_E_HIP, "mfx_dump_values_sharded: %s", hipGetErrorString(e));
  return rc;
}

// host threads the library may use for text formatting: min(hardware, cgroup quota, 64)
static thread_local unsigned t_sharers = 1;
extern "C" void mfx_host_threads_share(unsigned nsharers) { t_sharers = nsharers ? nsharers : 1; }
unsigned t_sharers_get() { return t_sharers; }

static unsigned host_threads_total();
unsigned mfx_host_threads() { return std::max(1u, host_threads_total() / t_sharers); }

static unsigned host_threads_total() {
  const char *e = getenv("MFX_HOST_THREADS");
  if (e && atoi(e) > 0) return (unsigned)atoi(e);
  unsigned n = std::thread::hardware_concurrency();
  if (n == 0) n = 1;
  if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[64], per[64];
    if (fscanf(f, "%63s %63s", q, per) == 2 && strcmp(q, "max") != 0 && atof(per) > 0) {
      unsigned lim = (unsigned)(atof(q) / atof(per));
      if (lim >= 1 && lim < n) n = lim;
    }
    fclose(f);
  }
  return std::min(n, 64u);
}

// Formats the lines of outputDump (merfin-dump.C:87-93) for positions
// [o, o+cnt) into `out`.  The text after the position depends only on the
// (readV, asmV) pair, so it is produced once per distinct pair by the very
// same printf("%.2f") the reference uses and then reused: the common pairs (read count < 256, assembly count < 16)
// from a table indexed by the pair, the others from a map.
namespace {
struct DumpTails {
  struct Small { char n = -1; char t[39]; };                // n: -1 = not made yet, 0 = no line for this pair
  std::vector<Small> lut;                                   // [rv < 256][av < 16]
  std::unordered_map<uint64_t, std::string> rest;
  const mfx_kparams &kp;
  explicit DumpTails(const mfx_kparams &k) : lut(256 * 16), kp(k) {}
  // the text after the position ("\t%.2f\t%.2f\t%.2f\n"), or n = 0 when all three values are zero
  int make(uint32_t rv, uint32_t av, char *buf, size_t cap) const {
    double readK, asmK, prob;
    mfx_getK(&kp, rv, av, &readK, &asmK, &prob);
    const double km = mfx_kmetric(readK, asmK);
    if (!((readK != 0.0) || (asmK != 0.0) || (km != 0.0))) return 0;
    return snprintf(buf, cap, "\t%.2f\t%.2f\t%.2f\n", readK, asmK, km);
  }
  const char *get(uint32_t rv, uint32_t av, size_t &n) {
    if (rv < 256u && av < 16u) {
      Small &e = lut[rv * 16u + av];
      if (e.n < 0) {
        char buf[128];
        const int m = make(rv, av, buf, sizeof(buf));
        if (m >= 0 && m < (int)sizeof(e.t)) { memcpy(e.t, buf, (size_t)m); e.n = (char)m; }
        else { n = 0; return nullptr; }                      // (cannot happen for these magnitudes; fall through to the map)
      }
      n = (size_t)e.n;
      return e.t;
    }
    const uint64_t key = ((uint64_t)rv << 32) | av;
    auto it = rest.find(key);
    if (it == rest.end()) {
      char buf[128];
      const int m = make(rv, av, buf, sizeof(buf));
      it = rest.emplace(key, std::string(buf, (size_t)std::max(m, 0))).first;
    }
    n = it->second.size();
    return it->second.data();
  }
};
}  // namespace

namespace {
struct RawBuf {                                             // a byte buffer that is never value-initialised (tens of MB per thread and chunk)
  char *p = nullptr;
  size_t cap = 0;
  char *data() { return p; }
  size_t size() const { return cap; }
  void resize(size_t n) {                                   // contents kept
    char *q = (char *)realloc(p, n);
    if (!q) throw std::bad_alloc();
    p = q; cap = n;
  }
  RawBuf() = default;
  RawBuf(const RawBuf &) = delete;
  RawBuf &operator=(const RawBuf &) = delete;
  ~RawBuf() { free(p); }
};
}  // namespace

static void dump_format_range(const mfx_kparams &kp, const char *name, size_t name_len, uint64_t o, uint64_t cnt,
                              const uint32_t *rv, const uint32_t *av, RawBuf &out, size_t &used) {
  DumpTails tails(kp);
  // the longest line: name, tab, 20 digits, tail (< 128)
  const size_t worst = name_len + 1 + 20 + 128;
  if (out.size() < cnt * 32 + worst) out.resize(cnt * 32 + worst);
  char *w = out.data(), *lim = out.data() + out.size() - worst;
  char num[24];
  for (uint64_t i = 0; i < cnt; ++i) {
    if (rv[i] == 0 && av[i] == 0) continue;            // readK = asmK = K* = 0: no line
    size_t tn = 0;
    const char *t = tails.get(rv[i], av[i], tn);
    if (tn == 0) continue;
    if (w > lim) {                                       // (lines longer than the estimate: long names)
      const size_t at = (size_t)(w - out.data());
      out.resize(out.size() * 2 + worst);
      w = out.data() + at;
      lim = out.data() + out.size() - worst;
    }
    uint64_t pos = o + i;
    int d = 0;
    do { num[d++] = (char)('0' + pos % 10); pos /= 10; } while (pos);
    memcpy(w, name, name_len);
    w += name_len;
    *w++ = '\t';
    while (d) *w++ = num[--d];
    memcpy(w, t, tn);
    w += tn;
  }
  used = (size_t)(w - out.data());
}

// positions per chunk: MFX_DUMP_CHUNK from 1 to 1 << 24 as given (the tests bring the chunk seam within reach of a small
// contig); unset, 0, malformed or larger: 1 << 24
static uint64_t dump_chunk() {
  const uint64_t dflt = 1ull << 24;
  const char *e = getenv("MFX_DUMP_CHUNK");
  if (!e || *e < '0' || *e > '9') return dflt;
  char *end = nullptr;
  errno = 0;
  const unsigned long long v = strtoull(e, &end, 10);
  if (errno || *end || v < 1 || v > dflt) return dflt;
  return (uint64_t)v;
}

// outputDump, merfin-dump.C:87-93: a line for every position where any of
// readK, asmK, K* is non-zero.  Values come from the GPU in 16 M-position
// chunks -- chunk i + 1 is looked up while chunk i is formatted and written --; host threads format disjoint sub-ranges and,
// for a plain file, write them themselves at the offsets the sizes of the ranges before them give (one writer moved 2.2 GB of
// text at 2.5 GB/s: 0.9 of the 1.06 s a config-2 dump took); a compressed output goes through its pipe in order.
// values(o, e, rv, av, &kasm, &kmissing) fills the (readV, asmV) pairs of positions [o, e): one evaluator or the shards of one index
template <class Values>
static int dump_contig_impl(const mfx_eval *ev, const mfx_seq *seq, uint32_t contig, const char *name,
                            const char *path, int append, uint64_t *kasm, uint64_t *kmissing, Values values) {
  const bool timing = getenv("MFX_DUMP_TIMING") != nullptr;
  auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  double t_values = 0, t_format = 0, t_write = 0;
  const bool plain = mfx_suffix_tool(path) == nullptr && !(getenv("MFX_DUMP_SERIAL") && atoi(getenv("MFX_DUMP_SERIAL")));
  mfx_file fh;
  FILE *f = nullptr;
  int fd = -1;
  uint64_t file_off = 0;
  if (plain) {
    fd = open(path, O_WRONLY | O_CREAT | O_CLOEXEC | (append ? 0 : O_TRUNC), 0666);
    if (fd < 0) return mfx_fail(MFX_E_IO, "cannot open '%s' for writing", path);
    if (append) { const off_t end = lseek(fd, 0, SEEK_END); file_off = end > 0 ? (uint64_t)end : 0; }
  } else {
    fh = mfx_open_writer(path, append != 0);
    f = fh.f;
    if (!f) return mfx_fail(MFX_E_IO, "cannot open '%s' for writing", path);
  }
  const uint64_t len = seq->len[contig];
  const uint64_t CH = dump_chunk();
  struct U32Buf { std::unique_ptr<uint32_t[]> p; uint32_t *data() { return p.get(); } } rvb[2], avb[2];     // (not value-initialised)
  for (int b = 0; b < 2; ++b) { rvb[b].p.reset(new uint32_t[std::min(len, CH) + 1]); avb[b].p.reset(new uint32_t[std::min(len, CH) + 1]); }
  mfx_kparams kp{ev->peak, ev->n_prob, ev->probK.data(), ev->probP.data()};
  const size_t name_len = strlen(name);
  const unsigned nthr = mfx_host_threads();
  std::vector<RawBuf> parts(nthr);
  std::vector<size_t> used(nthr, 0);
  uint64_t ka = 0, km = 0;
  int rc = MFX_OK;
  // the values of chunk c (positions [c * CH, ...)) into buffer c & 1, on a helper thread
  struct Fetch { std::thread th; int rc = MFX_OK; uint64_t a = 0, m = 0; std::string err; double dt = 0; } fetch;
  auto start_fetch = [&](uint64_t o) {
    fetch.rc = MFX_OK; fetch.a = fetch.m = 0;
    const int b = (int)((o / CH) & 1);
    fetch.th = std::thread([&, o, b]() {
      const double t0 = now();
      fetch.rc = values(o, std::min(len, o + CH), rvb[b].data(), avb[b].data(), &fetch.a, &fetch.m);
      if (fetch.rc) fetch.err = mfx_last_error();          // (errors are per thread: carried back to the caller's)
      fetch.dt = now() - t0;
    });
  };
  if (len) start_fetch(0);
  for (uint64_t o = 0; o < len && rc == MFX_OK; o += CH) {
    const uint64_t e = std::min(len, o + CH);
    const int b = (int)((o / CH) & 1);
    double t0 = now();
    fetch.th.join();
    t_values += now() - t0;
    if (fetch.rc) { rc = mfx_fail(fetch.rc, "%s", fetch.err.c_str()); break; }
    ka += fetch.a;
    km += fetch.m;
    if (e < len) start_fetch(e);
    const uint64_t cnt = e - o, per = (cnt + nthr - 1) / nthr;
    const uint32_t *rv = rvb[b].data(), *av = avb[b].data();
    t0 = now();
    std::atomic<bool> fmt_ok{true};
    {
      std::vector<std::thread> th;
      for (unsigned t = 0; t < nthr; ++t) {
        const uint64_t bb = std::min(cnt, t * per), n = std::min(cnt, bb + per) - bb;
        th.emplace_back([&, t, bb, n]() {
          try { dump_format_range(kp, name, name_len, o + bb, n, rv + bb, av + bb, parts[t], used[t]); }
          catch (const std::bad_alloc &) { used[t] = 0; fmt_ok = false; }
        });
      }
      for (auto &x : th) x.join();
    }
    t_format += now() - t0;
    if (!fmt_ok) { rc = mfx_fail(MFX_E_NOMEM, "out of host memory while formatting the dump of '%s'", name); break; }
    t0 = now();
    if (plain) {
      std::vector<uint64_t> at(nthr + 1, file_off);
      for (unsigned t = 0; t < nthr; ++t) at[t + 1] = at[t] + used[t];
      std::atomic<bool> wok{true};
      std::vector<std::thread> th;
      for (unsigned t = 0; t < nthr; ++t) {
        if (!used[t]) continue;
        th.emplace_back([&, t]() {
          const char *p = parts[t].p;
          size_t left = used[t];
          uint64_t off = at[t];
          while (left) {
            const ssize_t r = pwrite(fd, p, std::min<size_t>(left, 64u << 20), (off_t)off);
            if (r < 0 && errno == EINTR) continue;
            if (r <= 0) { wok = false; return; }
            p += r; left -= (size_t)r; off += (uint64_t)r;
          }
        });
      }
      for (auto &x : th) x.join();
      file_off = at[nthr];
      if (!wok) rc = mfx_fail(MFX_E_IO, "short write to '%s'", path);
    } else {
      for (unsigned t = 0; t < nthr; ++t)
        if (used[t] && fwrite(parts[t].data(), 1, used[t], f) != used[t]) {
          rc = mfx_fail(MFX_E_IO, "short write to '%s'", path);
          break;
        }
    }
    t_write += now() - t0;
  }
  if (fetch.th.joinable()) fetch.th.join();                 // (after an error: the look-ahead is waited for, nothing of it is used)
  if (plain) {
    if (close(fd) != 0 && rc == MFX_OK) rc = mfx_fail(MFX_E_IO, "writing '%s' failed", path);
  } else if (mfx_close(fh) && rc == MFX_OK) rc = mfx_fail(MFX_E_IO, "writing '%s' failed (stream error or the compressor exited with an error)", path);
  if (timing) fprintf(stderr, "-- dump of %s: waited for values %.3f s, format %.3f s, write %.3f s (%u threads%s)\n", name, t_values, t_format, t_write, nthr, plain ? ", positional writes" : "");
  if (kasm) *kasm = ka;
  if (kmissing) *kmissing = km;
  return rc;
}

extern "C" int mfx_dump_contig(mfx_eval *ev, const mfx_seq *seq, uint32_t contig, const char *name,
                               const char *path, int append, uint64_t *kasm, uint64_t *kmissing) {
  if (!ev || !seq || !name || !path) return mfx_fail(MFX_E_INVAL, "mfx_dump_contig: null argument");
  if (contig >= seq->ncontigs) return mfx_fail(MFX_E_INVAL, "mfx_dump_contig: contig %u out of range", contig);
  return dump_contig_impl(ev, seq, contig, name, path, append, kasm, kmissing,
                          [&](uint64_t o, uint64_t e, uint32_t *rv, uint32_t *av, uint64_t *a, uint64_t *m) {
                            return mfx_dump_values(ev, seq, contig, o, e, rv, av, a, m);
                          });
}

extern "C" int mfx_dump_contig_sharded(mfx_eval *const *evs, const mfx_seq *const *seqs, uint32_t nslots, uint32_t contig,
                                       const char *name, const char *path, int append, uint64_t *kasm, uint64_t *kmissing) {
  if (!evs || !seqs || nslots == 0 || !evs[0] || !seqs[0] || !name || !path)
    return mfx_fail(MFX_E_INVAL, "mfx_dump_contig_sharded: null argument");
  if (contig >= seqs[0]->ncontigs) return mfx_fail(MFX_E_INVAL, "mfx_dump_contig_sharded: contig %u out of range", contig);
  return dump_contig_impl(evs[0], seqs[0], contig, name, path, append, kasm, kmissing,
                          [&](uint64_t o, uint64_t e, uint32_t *rv, uint32_t *av, uint64_t *a, uint64_t *m) {
                            return mfx_dump_values_sharded(evs, seqs, nslots, contig, o, e, rv, av, a, m);
                          });
}
