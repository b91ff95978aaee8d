// mfx_stream.cpp -- the host -> device transport of an assembly that lives in HOST memory.
// Streamed -hist: the assembly arrives as HOST buffers (what loadSequence hands over, merfin.C:30-53) and its
// upload is overlapped with the evaluation -- SURVEY 8(d)'s timed region "first tile H2D start -> final reduced
// histogram on host".  The tiles are cut into chunks; chunk i's bytes travel on a copy stream while the -hist
// kernel of chunk i-1 runs on the compute stream (one event per chunk orders them), and the counts image comes
// back with one D2H copy at the end.  Buffers from mfx_host_alloc (pinned) are DMA'd in place; pageable buffers
// go through pinned staging buffers filled by host threads.
// mfx_seq_upload's packed transport (seq_upload_packed) is the same chunk plan, encoder and ring of staging buffers without the
// evaluation.  The arithmetic of both is mfx_stream_plan.h.
#include "mfx_host.h"
#include "mfx_histsum.h"
#include "mfx_kernels.h"
#include "mfx_pool.h"
#include "mfx_stream_plan.h"

#include <pthread.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <map>
#include <memory>

// A HIP call of a streamed run.  On failure the error is recorded and the function returns through the cleanup() of the place the macro
// is used in (StreamRun::cleanup, the lambda of mfx_hist_run_streamed): once host threads or streams work for the run, nothing returns past it.
#define STREAMED_HIP(call)                                                                                        \
  do {                                                                                                            \
    hipError_t e_ = (call);                                                                                       \
    if (e_ != hipSuccess) { const int rc_ = mfx_fail(MFX_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); cleanup(); return rc_; } \
  } while (0)

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

extern "C" void *mfx_host_alloc(size_t bytes) {
  void *p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    mfx_fail(MFX_E_NOMEM, "mfx_host_alloc: cannot pin %zu bytes of host memory", bytes);
    return nullptr;
  }
  return p;
}

extern "C" void mfx_host_free(void *p) {
  if (p) (void)hipHostFree(p);
}

static bool host_ptr_is_pinned(const void *p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return at.type == hipMemoryTypeHost;
}

// The CPUs of the NUMA node that holds `addr` (two-socket hosts: an encoder thread on the other socket reads the assembly over
// the inter-socket links).  false: unknown (no such call in this container, one node, too few of its CPUs allowed) -- no binding.
static bool cpus_near(const void *addr, cpu_set_t *out, int *node_out = nullptr) {
  const char *e = getenv("MFX_NUMA_BIND");
  if (e && atoi(e) == 0) return false;
  int node = -1;
  if (syscall(SYS_get_mempolicy, &node, nullptr, 0UL, const_cast<void *>(addr), 3UL /* MPOL_F_NODE | MPOL_F_ADDR */) != 0 || node < 0) return false;
  char path[96];
  snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
  FILE *f = fopen(path, "r");
  if (!f) return false;
  char buf[4096];
  const bool got = fgets(buf, sizeof(buf), f) != nullptr;
  fclose(f);
  if (!got) return false;
  cpu_set_t allowed, near;
  CPU_ZERO(&near);
  if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return false;
  for (char *p = buf; *p;) {                                  // "0-63,128-191"
    char *q;
    const long a = strtol(p, &q, 10);
    if (q == p) break;
    long b = a;
    if (*q == '-') { p = q + 1; b = strtol(p, &q, 10); }
    for (long c = a; c <= b && c < CPU_SETSIZE; ++c) if (CPU_ISSET(c, &allowed)) CPU_SET(c, &near);
    p = *q == ',' ? q + 1 : q;
    if (*q != ',' ) break;
  }
  if (node_out) *node_out = node;
  if ((unsigned)CPU_COUNT(&near) < std::max(1u, mfx_host_threads())) return false;
  if (CPU_COUNT(&near) == CPU_COUNT(&allowed)) return false;  // one node: nothing to choose
  *out = near;
  return true;
}

// Where the W encoder threads of a streamed run go.  A core reads memory through its CCD's link to the I/O die, and a few
// threads saturate one link (EPYC 9575F, tools/native/pack_bench.cpp: 8 threads in one CCD encode 55 GB/s of bases, 8 threads in 8
// CCDs 130-147 GB/s), so WHERE the scheduler happens to put the threads decides the rate of the whole pipeline: 16 threads that
// share two CCDs encode 99 GB/s, spread over the CCDs 145-193 GB/s.  MFX_PACK_PLACE:
//   spread (default) worker w is pinned to L3 domain w mod n of the source's NUMA node (every node if that is unknown), on the
//                    first hardware thread of its cores;   node  the CPUs of the source's node (the round-3 behaviour);
//   all              L3 domains of every node;   os  no binding
struct PackTopology {
  std::vector<std::vector<int>> l3_of_node[8];        // [node][domain] -> primary hardware threads
  cpu_set_t allowed;
  bool ok = false;
  PackTopology() {
    CPU_ZERO(&allowed);
    if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return;
    auto read_int = [](const char *p) { int v = -1; if (FILE *f = fopen(p, "r")) { if (fscanf(f, "%d", &v) != 1) v = -1; fclose(f); } return v; };
    std::map<std::pair<int, int>, std::vector<int>> dom;
    for (int c = 0; c < CPU_SETSIZE; ++c) {
      if (!CPU_ISSET(c, &allowed)) continue;
      char p[160];
      snprintf(p, sizeof(p), "/sys/devices/system/cpu/cpu%d/topology/thread_siblings_list", c);
      if (read_int(p) != c) continue;                  // a second hardware thread of its core
      snprintf(p, sizeof(p), "/sys/devices/system/cpu/cpu%d/cache/index3/id", c);
      const int l3 = read_int(p);
      int node = -1;
      for (int nd = 0; nd < 8 && node < 0; ++nd) {
        snprintf(p, sizeof(p), "/sys/devices/system/cpu/cpu%d/node%d", c, nd);
        if (access(p, F_OK) == 0) node = nd;
      }
      if (l3 < 0) continue;
      dom[{node < 0 ? 0 : node, l3}].push_back(c);
    }
    for (auto &kv : dom) l3_of_node[kv.first.first].push_back(kv.second);
    size_t n = 0;
    for (auto &v : l3_of_node) n += v.size();
    ok = n > 1;
  }
};
static const PackTopology &pack_topology() { static PackTopology t; return t; }

// the CPU set worker w of W runs on under `mode` (0 os, 1 node, 2 spread, 3 all); false: leave the thread where it is allowed
static bool pack_cpus(int mode, int node, const cpu_set_t *near, unsigned w, cpu_set_t *out) {
  const PackTopology &T = pack_topology();
  if (mode == 0) { *out = T.allowed; return CPU_COUNT(&T.allowed) > 0; }
  if (mode == 1) { if (near) { *out = *near; return true; } *out = T.allowed; return CPU_COUNT(&T.allowed) > 0; }
  if (!T.ok) { *out = T.allowed; return CPU_COUNT(&T.allowed) > 0; }
  std::vector<const std::vector<int> *> doms;
  if (mode == 2 && node >= 0 && node < 8) for (auto &d : T.l3_of_node[node]) doms.push_back(&d);
  if (doms.empty()) for (auto &nd : T.l3_of_node) for (auto &d : nd) doms.push_back(&d);
  CPU_ZERO(out);
  for (int c : *doms[w % doms.size()]) CPU_SET(c, out);
  return CPU_COUNT(out) > 0;
}

void mfx_pin_spread(unsigned w) {                      // (mfx_pool.h) the "all" placement, where the L3 domains are known
  const char *e = getenv("MFX_POOL_SPREAD");
  if (e && atoi(e) == 0) return;
  cpu_set_t mine;
  if (pack_topology().ok && pack_cpus(3, -1, nullptr, w, &mine)) (void)pthread_setaffinity_np(pthread_self(), sizeof(mine), &mine);
}

// ---- the two rates of a transport -------------------------------------------------------------------------------------------------
// scratch planes for W threads that encode `per` bases each (written: the scratch's pages exist before a clock starts)
static std::vector<std::vector<uint64_t>> encode_scratch(unsigned W, uint64_t per) {
  return std::vector<std::vector<uint64_t>>(W, std::vector<uint64_t>(per / 32 + per / 64 + 2, 1));
}
// the W threads of `pool` encode `per` bases each, all at once (they share the memory system), thread w those from `from + w * per`:
// GB of bases per second (0: no time passed)
static double encode_rate(WorkerPool *pool, unsigned W, const uint8_t *from, uint64_t per, std::vector<std::vector<uint64_t>> &sc) {
  auto run = [&](unsigned w) { mfx_pack_bases(from + (uint64_t)w * per, per, sc[w].data(), reinterpret_cast<uint32_t *>(sc[w].data() + per / 32 + 1)); };
  const auto t0 = std::chrono::steady_clock::now();
  pool->start(run); pool->wait();
  const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return dt > 0 ? (double)per * W / dt / 1e9 : 0.0;
}
// `reps` copies of m bytes of pinned host memory to `d` over `st`, each between two events, behind 1 MB that wakes the link up:
// the best one's GB/s (0: a call failed)
static double link_rate(uint8_t *d, const uint8_t *pinned_src, uint64_t m, hipStream_t st, int reps) {
  hipEvent_t a = nullptr, b = nullptr;
  double gbs = 0.0;
  bool ok = hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess && hipMemcpyAsync(d, pinned_src, 1u << 20, hipMemcpyHostToDevice, st) == hipSuccess;
  for (int rep = 0; rep < reps && ok; ++rep) {
    float ms = 0;
    ok = hipEventRecord(a, st) == hipSuccess && hipMemcpyAsync(d, pinned_src, m, hipMemcpyHostToDevice, st) == hipSuccess &&
         hipEventRecord(b, st) == hipSuccess && hipEventSynchronize(b) == hipSuccess;
    if (ok && hipEventElapsedTime(&ms, a, b) == hipSuccess && ms > 0) gbs = std::max(gbs, (double)m / (ms * 1e-3) / 1e9);
  }
  if (!ok) (void)hipGetLastError();
  if (a) (void)hipEventDestroy(a);
  if (b) (void)hipEventDestroy(b);
  return gbs;
}

// The two rates that decide how a streamed run's bases cross the link (StreamRun::choose_transport): what W host threads ENCODE (GB of
// bases per second, all of them at once: they share the memory system) and what the device's LINK moves from pinned host memory.
// Measured once per process and (W | device) on the caller's own buffers -- every thread encodes 4 MB of the first contig into a scratch of
// its own, 32 MB of it are copied to the device buffer they go to anyway -- ~1.5 ms together; MFX_STREAM_ENC_GBS / MFX_STREAM_LINK_GBS override.
static double stream_encode_gbs(WorkerPool *pool, unsigned W, const uint8_t *src, uint64_t n) {
  static std::mutex mu;
  static std::map<unsigned, double> cache;
  if (const char *e = getenv("MFX_STREAM_ENC_GBS")) if (atof(e) > 0) return atof(e);
  {
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(W);
    if (it != cache.end()) return it->second;
  }
  const uint64_t per = std::min<uint64_t>(4u << 20, n / std::max(1u, W) / 32 * 32);
  if (!pool || per < (1u << 16)) return 0.0;                  // too little to measure: no estimate
  auto sc = encode_scratch(W, per);
  // ONE pass over bases nobody has read yet (the tail of the contig: a second pass over the same 4 MB per thread would be served by the L3)
  const double gbs = encode_rate(pool, W, src + (n - (uint64_t)W * per) / 128 * 128, per, sc);
  std::lock_guard<std::mutex> lk(mu);
  cache[W] = gbs;
  return gbs;
}
static double stream_link_gbs(int device, uint8_t *d_dst, const uint8_t *pinned_src, uint64_t n, hipStream_t st) {
  static std::mutex mu;
  static std::map<int, double> cache;
  if (const char *e = getenv("MFX_STREAM_LINK_GBS")) if (atof(e) > 0) return atof(e);
  {
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(device);
    if (it != cache.end()) return it->second;
  }
  const uint64_t m = std::min<uint64_t>(32u << 20, n);
  if (m < (4u << 20)) return 0.0;
  const double gbs = link_rate(d_dst, pinned_src, m, st, 1);
  if (gbs > 0) { std::lock_guard<std::mutex> lk(mu); cache[device] = gbs; }
  return gbs;
}

// The two rates of the transport decision, measured on demand (bench.py's model of SURVEY 8(d)'s metric at N GPUs: a rank of N has
// host_threads / N encoders and a link of its own): `threads` host threads encoding `src` (pinned or not) at once, and -- src pinned --
// 256 MB of it over this device's link.  Nothing is cached.
extern "C" int mfx_diag_stream_rates(int device, const char *src, uint64_t n, uint32_t threads, double *enc_gbs, double *link_gbs) {
  if (!src || !enc_gbs || !link_gbs || threads == 0 || threads > 256) return mfx_fail(MFX_E_INVAL, "mfx_diag_stream_rates: bad argument");
  if (device < 0 || device >= mfx_device_count()) return mfx_fail(MFX_E_NODEVICE, "mfx_diag_stream_rates: device %d of %d", device, mfx_device_count());
  *enc_gbs = *link_gbs = 0.0;
  {
    WorkerPool pool(threads, true);                              // (spread over the L3 domains, as the run's own encoders are)
    // every pass reads bases no pass before it has read (a second pass over the same bytes would be served by the L3: 256 MB on the EPYC
    // of the measured boxes): up to three passes of `threads` x 32 MB, as far as n reaches; the best one counts
    const uint64_t per = std::min<uint64_t>(32u << 20, n / threads / 128 * 128);
    if (per >= (1u << 16)) {
      auto sc = encode_scratch(threads, per);
      const uint64_t passes = std::max<uint64_t>(1, std::min<uint64_t>(3, n / (per * threads)));
      for (uint64_t rep = 0; rep < passes; ++rep)
        *enc_gbs = std::max(*enc_gbs, encode_rate(&pool, threads, reinterpret_cast<const uint8_t *>(src) + rep * per * threads, per, sc));
    }
  }
  if (host_ptr_is_pinned(src) && n >= (4u << 20)) {
    DevGuard g(device);
    const uint64_t m = std::min<uint64_t>(256u << 20, n);
    uint8_t *d = nullptr;
    hipStream_t st = nullptr;
    if (hipMalloc((void **)&d, m) == hipSuccess && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess)
      *link_gbs = link_rate(d, reinterpret_cast<const uint8_t *>(src), m, st, 2);
    else (void)hipGetLastError();
    if (st) (void)hipStreamDestroy(st);
    if (d) (void)hipFree(d);
  }
  return MFX_OK;
}

// ---- the ring of staging buffers -----------------------------------------------------------------------------------------------------
// NB pinned staging buffers (code words, then validity words) go round: the W host threads of a pool encode chunk i+1 and i+2 into theirs
// while chunk i is on the bus.  Worker w encodes its share of the words of every chunk, in chunk order; the caller enqueues the chunks'
// copies in the same order and says when a copy has left its buffer.
namespace {
constexpr int NB = 3;
constexpr uint64_t STREAM_CH0 = 2048, STREAM_CH = 32768, UPLOAD_CH = 8192;      // tiles per chunk (mfx_stream_plan.h: stream_cuts, upload_cuts)

struct PackRing {
  std::atomic<int64_t> allowed{NB - 1};                     // chunks <= allowed may be packed (their staging buffer is free)
  std::atomic<bool> stop{false};
  std::vector<std::atomic<uint32_t>> done;                  // [chunk] packers that have encoded their share of it
  uint8_t *const *stage = nullptr;
  size_t stage_w = 0;                                       // words of a buffer
  WorkerPool *pool = nullptr;                               // set while its threads work for this ring
  void init(size_t nchunks, uint8_t *const *stage_, size_t stage_w_) {
    done = std::vector<std::atomic<uint32_t>>(nchunks);
    for (auto &d : done) d.store(0);
    stage = stage_;
    stage_w = stage_w_;
  }
  uint64_t *codes(size_t ci) const { return reinterpret_cast<uint64_t *>(stage[ci % NB]); }
  uint32_t *valid(size_t ci) const { return reinterpret_cast<uint32_t *>(stage[ci % NB] + stage_w * 8); }
  // every thread w of the pool calls share(w, ci) for the chunks in order, each once its buffer is free
  void start(WorkerPool *p, std::function<void(unsigned, size_t)> share) {
    pool = p;
    pool->start([this, share](unsigned w) {
      for (size_t ci = 0; ci < done.size(); ++ci) {
        while (allowed.load(std::memory_order_acquire) < (int64_t)ci) {
          if (stop.load()) return;
          std::this_thread::yield();
        }
        share(w, ci);
        done[ci].fetch_add(1, std::memory_order_release);
      }
    });
  }
  void wait_packed(size_t ci) const { while (done[ci].load(std::memory_order_acquire) < pool->W) std::this_thread::yield(); }
  // (ci >= 1) the copy of chunk ci-1, recorded in up[(ci-1) % NB], has left its buffer: chunk ci-1+NB may be packed into it
  hipError_t buffer_free_after(size_t ci, const hipEvent_t *up) {
    const hipError_t e = hipEventSynchronize(up[(ci - 1) % NB]);
    if (e == hipSuccess) allowed.store((int64_t)(ci - 1 + NB), std::memory_order_release);
    return e;
  }
  // packers that wait for a buffer give up; returns when none is at work (behind the last chunk: only the wait)
  void abort() {
    stop.store(true);
    if (pool) pool->wait();
    pool = nullptr;
  }
  ~PackRing() { abort(); }
};

// MFX_STREAM_TIMING=1: the phases of a streamed run on one line.  =2: also the timeline of every chunk (host clocks of the packers and of the
// enqueue loop, device events around its copy and behind its launch) -- what tools/stream_phases.py prints; costs a few events, never on by default
struct StreamTiming {
  struct ChunkTimes { double pack_first = 0, pack_last = 0, wait_buf = 0, enq = 0; hipEvent_t c0 = nullptr, c1 = nullptr, k1 = nullptr; };
  const int level = getenv("MFX_STREAM_TIMING") ? atoi(getenv("MFX_STREAM_TIMING")) : 0;
  const double t_begin = now_s();
  double mark[6] = {0, 0, 0, 0, 0, 0};
  std::vector<ChunkTimes> ct;
  hipEvent_t ev_base = nullptr;
  double t_base_host = 0;
  std::mutex mu;
  void chunks(size_t n) {
    if (level < 2) return;
    ct.resize(n);
    (void)hipEventCreate(&ev_base);
    for (auto &x : ct) { (void)hipEventCreate(&x.c0); (void)hipEventCreate(&x.c1); (void)hipEventCreate(&x.k1); }
  }
  double clock() const { return level >= 2 ? now_s() : 0.0; }
  void packed(size_t ci, double t_p0) {                       // one packer's share of chunk ci, begun at t_p0, is done
    if (level < 2) return;
    const double t_p1 = now_s();
    std::lock_guard<std::mutex> lk(mu);
    if (ct[ci].pack_first == 0 || t_p0 < ct[ci].pack_first) ct[ci].pack_first = t_p0;
    if (t_p1 > ct[ci].pack_last) ct[ci].pack_last = t_p1;
  }
  void base(hipStream_t cs) { if (level >= 2) { (void)hipEventRecord(ev_base, cs); (void)hipEventSynchronize(ev_base); t_base_host = now_s(); } }
  void buffer_free(size_t ci) { if (level >= 2) ct[ci].wait_buf = now_s(); }
  void copy_begin(size_t ci, hipStream_t cs) { if (level >= 2) { ct[ci].enq = now_s(); (void)hipEventRecord(ct[ci].c0, cs); } }
  void copy_end(size_t ci, hipStream_t cs) { if (level >= 2) (void)hipEventRecord(ct[ci].c1, cs); }
  void launched(size_t ci, hipStream_t kst) { if (level >= 2) (void)hipEventRecord(ct[ci].k1, kst); }
  void report(const std::vector<StreamChunk> &chunks, unsigned W, int place) const {
    if (level)
      fprintf(stderr, "[mfx stream] %zu chunks: setup %.2f ms, spawn %.2f, enqueue loop %.2f, drain %.2f, result %.2f, cleanup %.2f; total %.2f ms%s\n", chunks.size(),
              (mark[0] - t_begin) * 1e3, (mark[1] - mark[0]) * 1e3, (mark[2] - mark[1]) * 1e3, (mark[3] - mark[2]) * 1e3,
              (mark[4] - mark[3]) * 1e3, (mark[5] - mark[4]) * 1e3, (mark[5] - t_begin) * 1e3, place == 0 ? "; encoders unbound" : place == 1 ? "; encoders on the source's NUMA node" : place == 2 ? "; encoders spread over the L3 domains of the source's node" : "; encoders spread over all L3 domains");
    if (level < 2) return;
    // all times in ms since the function was entered; device times are placed on the host clock through ev_base
    fprintf(stderr, "[mfx stream] chunk   Mbases  pack:first..last   buf-wait   enqueue   copy:start..end   kernel-end   (ms since entry; %u packer threads)\n", W);
    for (size_t ci = 0; ci < chunks.size(); ++ci) {
      float a = 0, b2 = 0, k2 = 0;
      (void)hipEventElapsedTime(&a, ev_base, ct[ci].c0);
      (void)hipEventElapsedTime(&b2, ev_base, ct[ci].c1);
      (void)hipEventElapsedTime(&k2, ev_base, ct[ci].k1);
      const double off = (t_base_host - t_begin) * 1e3;
      fprintf(stderr, "[mfx stream] %5zu %8.1f %8.2f %8.2f %10.2f %9.2f %9.2f %8.2f %11.2f\n", ci, (chunks[ci].hi - chunks[ci].lo) / 1e6,
              (ct[ci].pack_first - t_begin) * 1e3, (ct[ci].pack_last - t_begin) * 1e3, (ct[ci].wait_buf - t_begin) * 1e3, (ct[ci].enq - t_begin) * 1e3,
              off + a, off + b2, off + k2);
    }
  }
  ~StreamTiming() {
    for (auto &x : ct) { (void)hipEventDestroy(x.c0); (void)hipEventDestroy(x.c1); (void)hipEventDestroy(x.k1); }
    if (ev_base) (void)hipEventDestroy(ev_base);
  }
};

// what a packed streamed run takes besides eval_run_resources, kept in the evaluator like those: the copy stream, the events of the staging
// buffers and of the kernel streams' hand-over, and (exc_entries > 0) the device lists of exceptional validity words
int stream_run_resources(mfx_eval *ev, size_t words, size_t exc_entries) {
  if (int rc = eval_run_resources(ev, words)) return rc;
  auto &R = ev->sr;
  if (!R.copy) MFX_HIP(hipStreamCreateWithFlags(&R.copy, hipStreamNonBlocking));
  for (auto &e : R.up) if (!e) MFX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  if (!R.kdone) MFX_HIP(hipEventCreateWithFlags(&R.kdone, hipEventDisableTiming));
  if (R.exc_cap < exc_entries) {
    for (auto &x : R.d_exc) { if (x) (void)hipFree(x); x = nullptr; }
    for (auto &x : R.d_exc) MFX_HIP(hipMalloc((void **)&x, exc_entries * 8));
    R.exc_cap = exc_entries;
  }
  return MFX_OK;
}

// The streamed -hist with the assembly crossing PCIe PACKED (0.375 B per base): host threads encode every chunk into
// the tile form (2-bit codes + validity bits, csrc/mfx_pack.cpp) while the previous chunk is on the bus and the one
// before is being evaluated; the kernel reads its tiles from the packed planes (mfx_tile_fill_packed).  One byte per
// base never reaches the device (seq->bases_stale; unpacked on demand by mfx_seq_ensure_ascii).
// part != nullptr: only the tiles [part->tl, part->th) are encoded, uploaded and evaluated (one device's share of a run over several:
// mfx_hist_run_streamed_multi / mfx_hist_run_streamed_range); the sequence object then holds that part only (mfx_seq::partial).
// One run: hist_run_streamed_packed calls the steps in the order they stand here.  A step that fails has cleaned up.
struct StreamRun {
  mfx_eval *const ev;
  mfx_seq *const seq;
  const char *const *const bases;
  const StreamPart *const part;
  StreamTiming tm;
  const size_t words;
  const uint64_t TL, TH, T;                                   // the tiles [TL, TH) of this run, T of them
  const bool whole;
  std::vector<StreamChunk> chunks;
  size_t STAGE_W = 0, EXC_TOTAL = 0;                          // words of a staging buffer; entries of the packers' lists behind it
  unsigned W = 1;                                             // packers
  bool sparse_valid = true, link_ascii = false;
  std::vector<uint32_t> nexc;                                 // exceptional words listed by packer w of chunk ci: nexc[ci * 64 + w]
  std::vector<std::atomic<uint32_t>> dense;                   // a packer ran out of room: the chunk's validity words go whole
  cpu_set_t near_cpus;
  int src_node = -1, place = 2;
  bool bind = false;
  bool own_image = true, want_digest = false;
  uint64_t *d_counts = nullptr;
  double *d_kover = nullptr;
  PackRing ring;                                              // (last: its threads read the members above)

  StreamRun(mfx_eval *ev_, mfx_seq *seq_, const char *const *bases_, const StreamPart *part_)
      : ev(ev_), seq(seq_), bases(bases_), part(part_), words(MFX_HIST_WORDS(ev_->nbins, seq_->ncontigs)), TL(part_ ? part_->tl : 0),
        TH(part_ ? part_->th : seq_->ntiles), T(TH - TL), whole(TL == 0 && TH == seq_->ntiles) {}

  void cleanup() {
    ring.abort();
    if (ev->sr.copy) (void)hipStreamSynchronize(ev->sr.copy);
    for (auto &k : ev->sr.kern) if (k) (void)hipStreamSynchronize(k);
  }
  int fail(int rc) { cleanup(); return rc; }
  size_t cap_w() const { return STAGE_W / (8 * (size_t)W) + 64; }      // entries of one packer's list
  uint64_t *exc_lists(int b) const { return reinterpret_cast<uint64_t *>(ev->h_pack[b] + STAGE_W * 12); }

  void plan() {
    chunks = stream_chunks(seq, TL, stream_cuts(T, STREAM_CH0, STREAM_CH), true);
    STAGE_W = stage_words(chunks, 131072);                    // words of the largest chunk, rounded up to 1 MB of them
    tm.chunks(chunks.size());
  }

  // the planes, the pinned staging buffers, the packers' pool; the sequence object says what it is about to hold
  int staging() {
    if (int rc = seq_alloc_planes(seq)) return fail(rc);      // (no valid base outside the uploads)
    // pinned staging (codes words, then validity words) belongs to the evaluator: pinning costs more than the evaluation
    if (ev->h_pack_words != STAGE_W) {
      for (auto &p : ev->h_pack) { if (p) (void)hipHostFree(p); p = nullptr; }
      ev->h_pack_words = STAGE_W;
    }
    // The validity plane crosses the link SPARSE: a word of it is all ones wherever 32 consecutive bases are ACGT, so a chunk sends
    // its code words and the few validity words that are not (contig ends, gaps, N runs); the plane's range is filled with ones on the
    // device and those are put in (mfx_k_valid_scatter): 0.25 instead of 0.375 bytes per base over PCIe, the bound of the streamed run.
    // Every packer lists the exceptional words of its share behind the staging buffer (room for 1/8 of its words: a chunk with more goes whole).
    const char *spv = getenv("MFX_STREAM_SPARSE_VALID");
    sparse_valid = !(spv && atoi(spv) == 0);
    EXC_TOTAL = STAGE_W / 8 + 64 * 64;                        // entries behind a staging buffer (up to 64 packers)
    for (int b = 0; b < NB && b < (int)chunks.size(); ++b)
      if (!ev->h_pack[b]) STREAMED_HIP(hipHostMalloc((void **)&ev->h_pack[b], STAGE_W * 12 + EXC_TOTAL * 8, hipHostMallocDefault));
    nexc.assign(chunks.size() * 64, 0);
    dense = std::vector<std::atomic<uint32_t>>(chunks.size());
    for (auto &d : dense) d.store(0);
    seq->bases_stale = true;
    seq->planes_ok = true;
    seq->digest = 0;                                           // new content
    seq->partial = !whole;
    seq->part_lo = TL;
    seq->part_hi = TH;
    W = std::max(1u, std::min(mfx_host_threads(), 64u));
    if (ev->pool && ev->pool->W != W) { delete ev->pool; ev->pool = nullptr; }
    if (!ev->pool) ev->pool = new WorkerPool(W);
    ring.init(chunks.size(), ev->h_pack, STAGE_W);
    return MFX_OK;
  }

  // TRANSPORT.  Host-packed (0.25-0.375 bytes per base over the link, the encoders' work in front of it) is the faster way while the
  // host threads THIS call has encode faster than its link moves plain bytes -- one process with the host's cores to itself: 150-190 GB/s
  // against 56.  A rank of N processes has 1/N of the cores but a link of its own: from N = 4 on (16-core quota) its threads are slower than
  // its link, and the run of the whole node is bound by the host's encoders whatever N.  Then the bases cross as they
  // are -- DMA straight out of the caller's pinned buffers, no host thread touches them -- and mfx_pack_kernel makes the planes on the
  // device (3 GB of bytes: 1.5 ms of its HBM); the evaluation is the same launches over the same planes, bit for bit.  Pinned sources
  // only (pageable ones would need a host copy as dear as the encoding).  MFX_STREAM_TRANSPORT=pack | ascii forces either.
  int choose_transport() {
    auto &R = ev->sr;
    bool all_pinned = seq->ncontigs > 0;
    for (uint32_t c = 0; c < seq->ncontigs && all_pinned; ++c) all_pinned = seq->len[c] == 0 || host_ptr_is_pinned(bases[c]);
    const char *tp = getenv("MFX_STREAM_TRANSPORT");
    if (tp && !strcmp(tp, "ascii")) link_ascii = all_pinned;
    else if (tp && !strcmp(tp, "pack")) link_ascii = false;
    else if (all_pinned && seq->ncontigs && seq->len[0] >= (32u << 20)) {
      if (int brc = seq_need_bases(seq)) return brc;
      if (!R.copy) MFX_HIP(hipStreamCreateWithFlags(&R.copy, hipStreamNonBlocking));
      const double enc = stream_encode_gbs(ev->pool, W, reinterpret_cast<const uint8_t *>(bases[0]), seq->len[0]);
      const double link = stream_link_gbs(ev->device, seq->d_bases, reinterpret_cast<const uint8_t *>(bases[0]), seq->len[0], R.copy);
      link_ascii = enc > 0 && link > 0 && enc < link;
      if (tm.level) fprintf(stderr, "[mfx stream] transport: %u host threads encode %.1f GB/s, the link moves %.1f GB/s -> %s\n", W, enc, link, link_ascii ? "plain bytes + device-side packing" : "host-packed planes");
    }
    if (link_ascii) if (int brc = seq_need_bases(seq)) return brc;
    return MFX_OK;
  }

  // the packers: worker w encodes its share of the words of every chunk, in chunk order (none when the bases cross the link as they are)
  void start_packers() {
    bind = seq->ncontigs && bases[0] && cpus_near(bases[0], &near_cpus, &src_node);      // the encoders run next to the memory they read
    if (const char *pp = getenv("MFX_PACK_PLACE")) place = !strcmp(pp, "os") ? 0 : !strcmp(pp, "node") ? 1 : !strcmp(pp, "all") ? 3 : 2;
    if (const char *nb = getenv("MFX_NUMA_BIND")) if (atoi(nb) == 0) place = 0;
    tm.mark[0] = now_s();
    if (!link_ascii) ring.start(ev->pool, [this](unsigned w, size_t ci) { pack_share(w, ci); });
    tm.mark[1] = now_s();
  }
  void pack_share(unsigned w, size_t ci) {
    cpu_set_t mine;
    if (ci == 0 && pack_cpus(place, src_node, bind ? &near_cpus : nullptr, w, &mine)) (void)pthread_setaffinity_np(pthread_self(), sizeof(mine), &mine);
    const double t_p0 = tm.clock();
    pack_chunk_share(seq, bases, chunks[ci], w, W, ring.codes(ci), ring.valid(ci));
    if (sparse_valid) {
      uint64_t w0, w1;
      chunk_share(chunks[ci], w, W, &w0, &w1);
      const int64_t n = list_valid_exceptions(ring.valid(ci), w0, w1, exc_lists((int)(ci % NB)) + (size_t)w * cap_w(), cap_w());
      if (n < 0) dense[ci].store(1, std::memory_order_relaxed);
      nexc[ci * 64 + w] = n < 0 ? 0 : (uint32_t)n;
    }
    tm.packed(ci, t_p0);
  }

  // streams, events, the counts image and its pinned mirror: created once per evaluator (while the packers start); then the clears
  int take_resources() {
    if (int rc = stream_run_resources(ev, words, sparse_valid ? EXC_TOTAL : 0)) return fail(rc);
    auto &R = ev->sr;
    hipStream_t ks = R.kern[0];
    own_image = !(part && part->d_counts);
    d_counts = own_image ? R.d_counts : part->d_counts;
    d_kover = own_image ? R.d_kover : part->d_kover;
    if (own_image) {
      STREAMED_HIP(hipMemsetAsync(d_counts, 0, words * sizeof(uint64_t), ks));
      STREAMED_HIP(hipMemsetAsync(d_kover, 0, sizeof(double), ks));
    }
    STREAMED_HIP(hipMemsetAsync(ev->d_tile_ctr, 0, 2 * sizeof(uint64_t), ks));
    STREAMED_HIP(ovf_reset_hip(ev, ks));
    STREAMED_HIP(hipEventRecord(R.kdone, ks));
    STREAMED_HIP(hipStreamWaitEvent(R.kern[1], R.kdone, 0));          // the second kernel stream starts behind the clears
    if (int rc = ensure_tile_partials(ev, T)) return fail(rc);
    tm.base(R.copy);
    return MFX_OK;
  }

  // the packers' lists of chunk ci, one behind the other, at the head of the (now free) validity words of its staging buffer; their entries
  size_t gather_exceptions(size_t ci, uint64_t *all) const {
    const uint64_t *lists = exc_lists((int)(ci % NB));
    size_t n = 0;
    for (unsigned w = 0; w < W; ++w) {
      const uint32_t m_ = nexc[ci * 64 + w];
      if (m_) memcpy(all + n, lists + (size_t)w * cap_w(), (size_t)m_ * 8);
      n += m_;
    }
    return n;
  }

  // chunk ci: its bases over the copy stream as soon as they are packed, its launch behind them on one of the two kernel streams
  int enqueue_chunk(size_t ci) {
    auto &R = ev->sr;
    const StreamChunk &c = chunks[ci];
    const int b = (int)(ci % NB);
    hipStream_t cs = R.copy;
    if (ci >= 1) STREAMED_HIP(ring.buffer_free_after(ci, R.up));
    tm.buffer_free(ci);
    if (!link_ascii) ring.wait_packed(ci);
    tm.copy_begin(ci, cs);
    if (link_ascii && c.hi > c.lo) {
      // the chunk's pieces by DMA out of the caller's pinned buffers (the gaps between contigs stay the buffer's zero bytes), then the
      // planes of its words on the device, behind the copies on the same stream; a word shared with the chunk before is rewritten with
      // the value it has (that chunk's kernel may still read it)
      for (const Piece &pc : c.pieces)
        STREAMED_HIP(hipMemcpyAsync(seq->d_bases + seq->off[pc.contig] + pc.pos, bases[pc.contig] + pc.pos, pc.n, hipMemcpyHostToDevice, cs));
      STREAMED_HIP(mfx_k_pack(seq->d_bases + c.lo, seq->d_codes + c.lo / 32, seq->d_valid + c.lo / 32, (c.hi - c.lo) / 32, cs));
    } else if (c.hi > c.lo) {
      const uint64_t nw = (c.hi - c.lo) / 32;
      STREAMED_HIP(hipMemcpyAsync(seq->d_codes + c.lo / 32, ring.codes(ci), nw * 8, hipMemcpyHostToDevice, cs));
      // the sparse form pays (8 bytes per listed word against 4 per word sent whole) only while fewer than half of the chunk's
      // validity words are exceptional; a chunk of short or gappy contigs goes whole
      size_t n_exc = 0;
      for (unsigned w = 0; w < W; ++w) n_exc += nexc[ci * 64 + w];
      if (sparse_valid && !dense[ci].load(std::memory_order_relaxed) && 2 * n_exc < nw) {
        uint64_t *all = reinterpret_cast<uint64_t *>(ring.valid(ci));
        const size_t n = gather_exceptions(ci, all);
        // A chunk that starts inside a contig begins with the MFX_ALIGN bases the previous chunk already sent as the halo of its last
        // tile, and that chunk's kernel may still be reading them (the copy stream does not wait for it): those words are left out of
        // the fill -- they hold their final values, and the listed ones among them are only rewritten with the same value.  Filling
        // them with ones first would let the running kernel see an N or a contig end behind the cut as valid bases for a moment.
        const uint64_t keep = (ci > 0 && c.pieces.front().pos) ? std::min<uint64_t>(nw, MFX_ALIGN / 32) : 0;   // (the first chunk of a part has nobody before it)
        if (nw > keep) STREAMED_HIP(hipMemsetAsync(seq->d_valid + c.lo / 32 + keep, 0xff, (nw - keep) * 4, cs));
        if (n) {
          STREAMED_HIP(hipMemcpyAsync(R.d_exc[b], all, n * 8, hipMemcpyHostToDevice, cs));
          STREAMED_HIP(mfx_k_valid_scatter(seq->d_valid + c.lo / 32, R.d_exc[b], (uint32_t)n, cs));
        }
      } else {
        STREAMED_HIP(hipMemcpyAsync(seq->d_valid + c.lo / 32, ring.valid(ci), nw * 4, hipMemcpyHostToDevice, cs));
      }
    }
    tm.copy_end(ci, cs);
    STREAMED_HIP(hipEventRecord(R.up[b], cs));
    // two kernel streams (and tile counters) alternate: the first blocks of a launch fill the CUs the previous launch's
    // last blocks leave behind, instead of waiting for its tail
    hipStream_t kst = R.kern[ci & 1];
    STREAMED_HIP(hipStreamWaitEvent(kst, R.up[b], 0));
    if (int rc = hist_launch(ev, seq, c.t0, c.t1, 0, 1, 0, d_counts, d_kover, kst, T, (int)(ci & 1), TL)) return fail(rc);
    tm.launched(ci, kst);
    return MFX_OK;
  }

  // behind the last chunk: the digest of what was uploaded, the sum of the tiles' koverCpy, the image back on the host
  int drain() {
    auto &R = ev->sr;
    hipStream_t cs = R.copy, ks = R.kern[0];
    uint64_t *const h_img = R.h_img;
    tm.mark[2] = now_s();
    // a sequence-only index answers for the k-mers of ONE sequence: the content digest of what was just uploaded is taken on
    // the copy stream, behind the last chunk and under the last launches, and compared before the result is handed out
    // (a part cannot be checked: its digest is not the sequence's; the caller of the parts vouches for the sequence)
    want_digest = whole && ev->ix->seq_only && ev->ix->seq_digest != 0;
    if (want_digest) {
      uint64_t *d_dig = reinterpret_cast<uint64_t *>(R.d_kover + 1);      // the evaluator's own word (eval_run_resources), never the caller's one-double buffer of a range run
      STREAMED_HIP(hipMemsetAsync(d_dig, 0, sizeof(uint64_t), cs));
      STREAMED_HIP(mfx_k_seq_digest(nullptr, seq->d_codes, seq->d_valid, seq->buf_bytes / 32, d_dig, cs));
      STREAMED_HIP(hipMemcpyAsync(h_img + words + 1, d_dig, sizeof(uint64_t), hipMemcpyDeviceToHost, cs));
    }
    STREAMED_HIP(hipEventRecord(R.kdone, R.kern[1]));
    STREAMED_HIP(hipStreamWaitEvent(ks, R.kdone, 0));
    if (T) STREAMED_HIP(mfx_k_sum_tile_partials(ev->d_tile_partials, T, d_kover, ev->d_tile_ctr, ks, ev->ix->wide() ? 0 : 1));
    if (own_image) {
      STREAMED_HIP(hipMemcpyAsync(h_img, d_counts, words * sizeof(uint64_t), hipMemcpyDeviceToHost, ks));
      STREAMED_HIP(hipMemcpyAsync(h_img + words, d_kover, sizeof(double), hipMemcpyDeviceToHost, ks));
    }
    STREAMED_HIP(hipStreamSynchronize(ks));
    if (want_digest) STREAMED_HIP(hipStreamSynchronize(cs));
    if (part && part->chunk_sums) {
      // the first-level sums behind the (tile, wave) values: what mfx_sum_partials_kernel added up; the caller adds the parts' in the same order
      const uint64_t nv = T * (MFX_BLOCK / 64), nch = (nv + 4095) / 4096;
      part->chunk_sums->assign(nch, 0.0);
      if (nch) STREAMED_HIP(hipMemcpy(part->chunk_sums->data(), ev->d_tile_partials + nv, nch * sizeof(double), hipMemcpyDeviceToHost));
    }
    tm.mark[3] = now_s();
    return MFX_OK;
  }

  int result(mfx_hist_result *out) {
    const uint64_t *h_img = ev->sr.h_img;
    if (want_digest) {
      seq_digest_finish(seq, h_img[words + 1]);
      if (int rc = mfx_check_seq_of_index(ev->ix, seq, "-hist (streamed)")) return fail(rc);
    }
    double kover;
    memcpy(&kover, h_img + words, sizeof(double));
    const bool want_result = !part || (part->want_result && own_image);
    int rc = MFX_OK;
    if (want_result) rc = mfx_hist_result_from_counts(ev->nbins, h_img, kover, seq->ncontigs, out);
    const uint64_t novf = own_image ? h_img[mfx_histsum::novf(ev->nbins)] : 0;
    tm.mark[4] = now_s();
    cleanup();
    tm.mark[5] = now_s();
    tm.report(chunks, W, place);
    if (rc || !want_result) return rc;
    rc = result_take_overflow(ev, novf, out);
    if (rc) mfx_hist_result_free(out);
    return rc;
  }
};
}  // namespace

int hist_run_streamed_packed(mfx_eval *ev, mfx_seq *seq, const char *const *bases, mfx_hist_result *out, const StreamPart *part) {      // StreamPart: mfx_host.h
  DevGuard g(ev->device);
  StreamRun run(ev, seq, bases, part);
  run.plan();
  int rc = run.staging();
  if (!rc) rc = run.choose_transport();
  if (rc) return rc;
  run.start_packers();
  rc = run.take_resources();
  for (size_t ci = 0; ci < run.chunks.size() && !rc; ++ci) rc = run.enqueue_chunk(ci);
  if (!rc) rc = run.drain();
  return rc ? rc : run.result(out);
}

// mfx_seq_upload's transport: the same encoder and chunking as the streamed -hist, without the evaluation -- three small
// pinned buffers (32 M bases = 12 MB each: pinning costs 0.4 ms per MB, the old 2 x 64 MB of bytes cost 50 ms before
// the first base moved), the host threads encode chunk i+1 and i+2 while chunk i is on the bus.
int seq_upload_packed(mfx_seq *seq, const char *const *bases) {
  const bool timing = getenv("MFX_UPLOAD_TIMING") != nullptr;
  double tm[5] = {now_s(), 0, 0, 0, 0};
  const std::vector<StreamChunk> chunks = stream_chunks(seq, 0, upload_cuts(seq->ntiles, UPLOAD_CH), false);
  tm[1] = now_s();
  int rc = seq_alloc_planes(seq);
  if (rc) return rc;
  seq->bases_stale = true;
  seq->planes_ok = true;
  seq->digest = 0;
  seq->partial = false;
  if (chunks.empty()) return MFX_OK;
  tm[2] = now_s();
  const size_t STAGE_W = stage_words(chunks, 4096);
  uint8_t *stage[NB] = {nullptr, nullptr, nullptr};
  hipEvent_t up[NB] = {nullptr, nullptr, nullptr};
  hipStream_t cs = nullptr;
  const unsigned W = std::max(1u, std::min(mfx_host_threads(), 64u));
  std::unique_ptr<WorkerPool> pool;
  PackRing ring;
  bool ok = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) == hipSuccess;
  for (int b = 0; b < NB && b < (int)chunks.size() && ok; ++b)
    ok = hipHostMalloc((void **)&stage[b], STAGE_W * 12, hipHostMallocDefault) == hipSuccess &&
         hipEventCreateWithFlags(&up[b], hipEventDisableTiming) == hipSuccess;
  ring.init(chunks.size(), stage, STAGE_W);
  tm[3] = now_s();
  if (ok) {
    // (not spread over the L3 domains: 3 Gb are encoded + copied in 0.024-0.034 s as the threads fall, 0.034-0.070 s pinned; what an upload costs
    // is its device buffers -- 0.05-0.15 s for 3 GB: profiles/r04_cli_startup_1gb.txt)
    pool.reset(new WorkerPool(W));
    ring.start(pool.get(), [&](unsigned w, size_t ci) { pack_chunk_share(seq, bases, chunks[ci], w, W, ring.codes(ci), ring.valid(ci)); });
    for (size_t ci = 0; ci < chunks.size() && ok; ++ci) {
      const StreamChunk &c = chunks[ci];
      if (ci >= 1) ok = ring.buffer_free_after(ci, up) == hipSuccess;
      if (!ok) break;
      ring.wait_packed(ci);
      const uint64_t nw = (c.hi - c.lo) / 32;
      ok = hipMemcpyAsync(seq->d_codes + c.lo / 32, ring.codes(ci), nw * 8, hipMemcpyHostToDevice, cs) == hipSuccess &&
           hipMemcpyAsync(seq->d_valid + c.lo / 32, ring.valid(ci), nw * 4, hipMemcpyHostToDevice, cs) == hipSuccess &&
           hipEventRecord(up[ci % NB], cs) == hipSuccess;
    }
    ring.abort();
    if (hipStreamSynchronize(cs) != hipSuccess) ok = false;
  }
  tm[4] = now_s();
  for (int b = 0; b < NB; ++b) { if (stage[b]) (void)hipHostFree(stage[b]); if (up[b]) (void)hipEventDestroy(up[b]); }
  if (cs) (void)hipStreamDestroy(cs);
  if (timing)
    fprintf(stderr, "-- packed upload: chunk plan %.3f s, planes %.3f, pinned staging + stream %.3f, encode + copy %.3f (%u threads, %zu chunks), release %.3f\n",
            tm[1] - tm[0], tm[2] - tm[1], tm[3] - tm[2], tm[4] - tm[3], W, chunks.size(), now_s() - tm[4]);
  return ok ? MFX_OK : mfx_fail(MFX_E_HIP, "packed upload of the sequence failed: %s", hipGetErrorString(hipGetLastError()));
}

extern "C" int mfx_hist_run_streamed(mfx_eval *ev, mfx_seq *seq, const char *const *bases, mfx_hist_result *out) {
  if (!ev || !seq || !out || (seq->ncontigs && !bases)) return mfx_fail(MFX_E_INVAL, "mfx_hist_run_streamed: null argument");
  if (ev->device != seq->device) return mfx_fail(MFX_E_INVAL, "evaluator and sequence live on different devices");
  {
    // default: the assembly crosses the bus packed; MFX_STREAM_ASCII=1 (and the 128-bit k-mer kernels) send one byte per base
    const char *asc = getenv("MFX_STREAM_ASCII");
    if (!ev->ix->wide() && !(asc && atoi(asc))) return hist_run_streamed_packed(ev, seq, bases, out);
  }
  DevGuard g(ev->device);
  if (int brc = seq_need_bases(seq)) return brc;
  seq->bases_stale = false;                                 // this path writes d_bases
  seq->planes_ok = false;
  seq->digest = 0;
  seq->partial = false;
  const size_t words = MFX_HIST_WORDS(ev->nbins, seq->ncontigs);
  const uint64_t T = seq->ntiles;
  const uint64_t CH = 16384;                                // tiles per chunk: 64 MB of bases
  const size_t STAGE = (size_t)CH * (MFX_TILE + 2 * MFX_ALIGN) + MFX_TILE;   // worst case: every tile its own contig
  DevBuf<uint64_t> dc;
  DevBuf<double> dk;
  uint64_t *h_img = nullptr;                                // pinned: counts image + koverCpy
  // the pinned staging buffers (pageable sources only) belong to the evaluator: pinning 2 x 71 MB costs ~60 ms, more
  // than the whole evaluation of 3 Gb, so it is paid once per evaluator, not per call
  if (ev->h_stage_bytes != STAGE) {
    for (auto &p : ev->h_stage) { if (p) (void)hipHostFree(p); p = nullptr; }
    ev->h_stage_bytes = STAGE;
  }
  uint8_t **stage = ev->h_stage;
  hipStream_t cs = nullptr, ks = nullptr;
  hipEvent_t up[2] = {nullptr, nullptr}, staged[2] = {nullptr, nullptr};
  int rc = MFX_OK;
  auto cleanup = [&]() {
    if (cs) (void)hipStreamSynchronize(cs);
    if (ks) (void)hipStreamSynchronize(ks);
    for (int i = 0; i < 2; ++i) {
      if (up[i]) (void)hipEventDestroy(up[i]);
      if (staged[i]) (void)hipEventDestroy(staged[i]);
    }
    if (h_img) (void)hipHostFree(h_img);
    if (cs) (void)hipStreamDestroy(cs);
    if (ks) (void)hipStreamDestroy(ks);
  };
  STREAMED_HIP(dc.alloc(words));
  STREAMED_HIP(dk.alloc(1));
  STREAMED_HIP(hipHostMalloc((void **)&h_img, (words + 1) * sizeof(uint64_t), hipHostMallocDefault));
  STREAMED_HIP(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
  STREAMED_HIP(hipStreamCreateWithFlags(&ks, hipStreamNonBlocking));
  for (int i = 0; i < 2; ++i) {
    STREAMED_HIP(hipEventCreateWithFlags(&up[i], hipEventDisableTiming));
    STREAMED_HIP(hipEventCreateWithFlags(&staged[i], hipEventDisableTiming));
  }
  STREAMED_HIP(hipMemsetAsync(dc.p, 0, words * sizeof(uint64_t), ks));
  STREAMED_HIP(hipMemsetAsync(dk.p, 0, sizeof(double), ks));
  STREAMED_HIP(hipMemsetAsync(ev->d_tile_ctr, 0, sizeof(uint64_t), ks));
  STREAMED_HIP(ovf_reset_hip(ev, ks));
  if ((rc = ensure_tile_partials(ev, T)) != MFX_OK) { cleanup(); return rc; }
  std::vector<char> pinned(seq->ncontigs);
  for (uint32_t c = 0; c < seq->ncontigs; ++c) pinned[c] = seq->len[c] && host_ptr_is_pinned(bases[c]);
  std::vector<Piece> pieces;
  bool stage_busy[2] = {false, false};
  for (uint64_t t0 = 0, ci = 0; t0 < T; t0 += CH, ++ci) {
    const uint64_t t1 = std::min(T, t0 + CH);
    const int b = (int)(ci & 1);
    chunk_pieces(seq, t0, t1, pieces);
    bool direct = pieces.size() <= 64;                       // many small contigs: one assembled copy instead of many tiny ones
    for (const Piece &pc : pieces) direct = direct && pinned[pc.contig];
    if (direct) {
      for (const Piece &pc : pieces)
        STREAMED_HIP(hipMemcpyAsync(seq->d_bases + seq->off[pc.contig] + pc.pos, bases[pc.contig] + pc.pos, pc.n, hipMemcpyHostToDevice, cs));
    } else if (!pieces.empty()) {
      if (!stage[b]) STREAMED_HIP(hipHostMalloc((void **)&stage[b], STAGE, hipHostMallocDefault));
      if (stage_busy[b]) STREAMED_HIP(hipEventSynchronize(staged[b]));   // its previous copy has left the buffer
      // the staging buffer mirrors the device range [lo, hi) of this chunk; gaps between contigs stay non-ACGT
      const uint64_t lo = seq->off[pieces.front().contig] + pieces.front().pos;
      const uint64_t hi = seq->off[pieces.back().contig] + pieces.back().pos + pieces.back().n;
      if (hi - lo > STAGE) { rc = mfx_fail(MFX_E_INVAL, "mfx_hist_run_streamed: chunk of %lu bytes exceeds the staging buffer", (unsigned long)(hi - lo)); cleanup(); return rc; }
      uint64_t filled = lo;
      for (const Piece &pc : pieces) {
        const uint64_t at = seq->off[pc.contig] + pc.pos;
        if (at > filled) memset(stage[b] + (filled - lo), 0, at - filled);
        par_memcpy(stage[b] + (at - lo), bases[pc.contig] + pc.pos, pc.n);
        filled = at + pc.n;
      }
      STREAMED_HIP(hipMemcpyAsync(seq->d_bases + lo, stage[b], hi - lo, hipMemcpyHostToDevice, cs));
      STREAMED_HIP(hipEventRecord(staged[b], cs));
      stage_busy[b] = true;
    }
    STREAMED_HIP(hipEventRecord(up[b], cs));
    STREAMED_HIP(hipStreamWaitEvent(ks, up[b], 0));
    rc = hist_launch(ev, seq, t0, t1, 0, 1, 0, dc.p, dk.p, ks, T);
    if (rc) { cleanup(); return rc; }
  }
  if (T) STREAMED_HIP(mfx_k_sum_tile_partials(ev->d_tile_partials, T, dk.p, ev->d_tile_ctr, ks, ev->ix->wide() ? 0 : 1));
  STREAMED_HIP(hipMemcpyAsync(h_img, dc.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, ks));
  STREAMED_HIP(hipMemcpyAsync(h_img + words, dk.p, sizeof(double), hipMemcpyDeviceToHost, ks));
  STREAMED_HIP(hipStreamSynchronize(ks));
  double kover;
  memcpy(&kover, h_img + words, sizeof(double));
  if ((rc = mfx_check_seq_of_index(ev->ix, seq, "-hist (streamed)")) != MFX_OK) { cleanup(); return rc; }
  rc = mfx_hist_result_from_counts(ev->nbins, h_img, kover, seq->ncontigs, out);
  const uint64_t novf = h_img[mfx_histsum::novf(ev->nbins)];
  cleanup();
  if (rc) return rc;
  rc = result_take_overflow(ev, novf, out);
  if (rc) mfx_hist_result_free(out);
  return rc;
}
#undef STREAMED_HIP
