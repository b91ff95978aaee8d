// mfx_seq.cpp -- mfx_seq, the assembly on the device: layout, upload, digest, the packed planes.
#include "mfx_host.h"
#include "mfx_kernels.h"
#include "mfx_stream_plan.h"

#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <thread>
#include <vector>

// ---------------------------------------------------------------------------
// sequences
// ---------------------------------------------------------------------------
static mfx_seq *seq_layout(int device, const uint64_t *lens, uint32_t ncontigs) {
  mfx_seq *s = new mfx_seq;
  s->device = device;
  seq_layout_fill(s, lens, ncontigs);                                 // mfx_stream_plan.h
  return s;
}

// One byte per base (mfx_seq::d_bases) is what the 128-bit kernels, -dump, the router and the variant modes read; a sequence
// that arrives packed and is only ever counted and evaluated by the k <= 31 -hist kernels never needs it (3 GB for a human assembly,
// 0.05-0.15 s of its upload): it is made on first use (mfx_seq_ensure_ascii).
int seq_need_bases(mfx_seq *s) {
  if (s->d_bases) return MFX_OK;
  MFX_HIP(hipMalloc((void **)&s->d_bases, s->buf_bytes));
  MFX_HIP(mfx_memset_now(s->d_bases, 0, s->buf_bytes));                    // byte 0 is not ACGT: separators + padding
  return MFX_OK;
}

static int seq_alloc(mfx_seq *s, bool with_bases = true) {
  if (with_bases) if (int rc = seq_need_bases(s)) return rc;
  size_t nc = s->ncontigs ? s->ncontigs : 1;
  MFX_HIP(hipMalloc((void **)&s->d_contig_off, nc * sizeof(uint64_t)));
  MFX_HIP(hipMalloc((void **)&s->d_contig_len, nc * sizeof(uint64_t)));
  MFX_HIP(hipMalloc((void **)&s->d_tile_start, (nc + 1) * sizeof(uint64_t)));
  if (s->ncontigs) {
    MFX_HIP(hipMemcpy(s->d_contig_off, s->off.data(), s->ncontigs * sizeof(uint64_t), hipMemcpyHostToDevice));
    MFX_HIP(hipMemcpy(s->d_contig_len, s->len.data(), s->ncontigs * sizeof(uint64_t), hipMemcpyHostToDevice));
  }
  MFX_HIP(hipMemcpy(s->d_tile_start, s->tile_start.data(), (s->ncontigs + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
  {
    std::vector<uint32_t> tc((size_t)s->ntiles);
    for (uint32_t c = 0; c < s->ncontigs; ++c)
      std::fill(tc.begin() + (size_t)s->tile_start[c], tc.begin() + (size_t)s->tile_start[c + 1], c);
    MFX_HIP(hipMalloc((void **)&s->d_tile_contig, (tc.size() ? tc.size() : 1) * sizeof(uint32_t)));
    if (!tc.empty()) MFX_HIP(hipMemcpy(s->d_tile_contig, tc.data(), tc.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  return MFX_OK;
}

// A packed upload (mfx_hist_run_streamed) leaves the sequence in its packed planes only; the kernels that read one byte
// per base get them unpacked here, once, on first use.
// What a sequence makes on first use -- its bytes per base, its packed planes, its content digest -- is made under this lock:
// N slots that share a device share its mfx_seq (merfin -dump -devices 0,0,0,0: four threads ask one sequence for its bytes at
// once; unguarded, one thread's fill of the fresh buffer wiped what another had just unpacked and that slot dumped empty contigs).

int mfx_seq_partial_error(const mfx_seq *s, const char *who) {
  return mfx_fail(MFX_E_INVAL, "%s: the sequence object holds only the tiles [%lu, %lu) of its %lu (the part one device evaluated in a streamed run over "
                  "several); upload the sequence whole", who, (unsigned long)s->part_lo, (unsigned long)s->part_hi, (unsigned long)s->ntiles);
}

int mfx_seq_ensure_ascii(const mfx_seq *cs) {
  if (cs && cs->partial) return mfx_seq_partial_error(cs, "unpacking the sequence");
  std::lock_guard<std::mutex> lazy(cs->lazy_mu);
  if (!cs->bases_stale && cs->d_bases) return MFX_OK;
  mfx_seq *s = const_cast<mfx_seq *>(cs);
  DevGuard g(s->device);
  if (int rc = seq_need_bases(s)) return rc;
  if (!s->bases_stale) return MFX_OK;                       // (a sequence that holds nothing yet: all bytes 0)
  MFX_HIP(mfx_k_unpack(s->d_codes, s->d_valid, s->d_bases, s->buf_bytes / 32, nullptr));
  MFX_HIP(hipDeviceSynchronize());
  s->bases_stale = false;
  return MFX_OK;
}

// h: the device's sum over the words (mfx_seq_digest_kernel)
void seq_digest_finish(const mfx_seq *s, uint64_t h) {
  for (uint32_t c = 0; c < s->ncontigs; ++c) h = (h ^ s->len[c]) * 0x100000001B3ULL + c;       // the contig structure
  const uint32_t f = (uint32_t)(h ^ (h >> 32));
  s->digest = f ? f : 1u;
}

int mfx_seq_digest32(const mfx_seq *s, uint32_t *out) {
  if (s->partial) return mfx_seq_partial_error(s, "the sequence's content digest");
  std::lock_guard<std::mutex> lazy(s->lazy_mu);
  if (s->digest == 0) {
    DevGuard g(s->device);
    uint64_t *d = nullptr, h = 0;
    MFX_HIP(hipMalloc((void **)&d, sizeof(uint64_t)));
    hipError_t e = mfx_memset_now(d, 0, sizeof(uint64_t));
    const bool planes = s->planes_ok || s->bases_stale;
    if (!planes && !s->d_bases) { (void)hipFree(d); if (int rc = seq_need_bases(const_cast<mfx_seq *>(s))) return rc; MFX_HIP(hipMalloc((void **)&d, sizeof(uint64_t))); e = mfx_memset_now(d, 0, sizeof(uint64_t)); }
    if (e == hipSuccess) e = mfx_k_seq_digest(s->d_bases, planes ? s->d_codes : nullptr, planes ? s->d_valid : nullptr, s->buf_bytes / 32, d, nullptr);
    if (e == hipSuccess) e = hipMemcpy(&h, d, sizeof(h), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return mfx_fail(MFX_E_HIP, "sequence digest failed: %s", hipGetErrorString(e));
    seq_digest_finish(s, h);
  }
  *out = s->digest;
  return MFX_OK;
}

thread_local bool t_mfx_path_lookup = false;     // set by the variant modes around the lookups of THEIR path text (mfx_variants.cpp)
int mfx_check_seq_of_index(const mfx_index *ix, const mfx_seq *s, const char *who) {
  if (!ix->seq_only || ix->seq_digest == 0) return MFX_OK;
  if (ix->paths_token) {
    if (t_mfx_path_lookup) return MFX_OK;
    return mfx_fail(MFX_E_INVAL, "%s: this index holds the k-mers of a variant call set's PATHS (mfx_index_claim_paths) and answers the variant modes of that "
                    "call set only; build the index from the sequence (mfx_index_create_for_seq) or use a full index", who);
  }
  uint32_t d = 0;
  if (int rc = mfx_seq_digest32(s, &d)) return rc;
  if (d != ix->seq_digest)
    return mfx_fail(MFX_E_INVAL, "%s: this sequence-only index holds the k-mers of ANOTHER sequence (content digest %08x, this one %08x): "
                    "k-mers it never claimed would read as absent; build the index from this sequence (mfx_index_create_for_seq + "
                    "mfx_index_count_asm / mfx_index_claim_seq) or use a full index", who, ix->seq_digest, d);
  return MFX_OK;
}

// A sequence that has just been copied into d_bases (the library's own copy: nobody rewrites it) gets its packed planes here, once
// (mfx_seq_planes_once, mfx_internal.h): the resident -hist of 3 Gb read 3.05 GB of bytes and spent ~12 of its 200 wave instructions per
// k-mer encoding them, on every launch.  MFX_SEQ_PACK=0: the sequence stays one byte per base (A/B; docs/KNOBS.md).  The object is
// not shared yet: no lock.  Never fails -- without room for the planes the sequence is evaluated from its bytes.
static void seq_pack_resident(mfx_seq *s) {
  const char *e = getenv("MFX_SEQ_PACK");
  if ((e && atoi(e) == 0) || !s->d_bases) return;
  const bool timing = getenv("MFX_UPLOAD_TIMING") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  const uint64_t pw = seq_plane_words(s);
  const bool ok = mfx_seq_planes_once(
      s, pw,
      [](void **p, size_t bytes) { const bool got = hipMalloc(p, bytes) == hipSuccess; if (!got) { *p = nullptr; (void)hipGetLastError(); } return got; },
      [](void *p) { (void)hipFree(p); },
      [pw](mfx_seq *q) {
        const bool done = mfx_memset_now(q->d_valid, 0, pw * sizeof(uint32_t)) == hipSuccess &&              // no valid base behind the sequence
                          mfx_memset_now(q->d_codes, 0, pw * sizeof(uint64_t)) == hipSuccess &&
                          mfx_k_pack(q->d_bases, q->d_codes, q->d_valid, q->buf_bytes / 32, nullptr) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
        if (!done) (void)hipGetLastError();
        return done;
      });
  if (timing)
    fprintf(stderr, "-- resident sequence: packed planes %s, %.3f s (%.1f MB)\n", ok ? "made" : "NOT made (evaluated from its bytes)",
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), pw * 12 / 1e6);
}

extern "C" mfx_seq *mfx_seq_upload(int device, const char *const *bases, const uint64_t *lens, uint32_t ncontigs) {
  if ((ncontigs && (!bases || !lens)) || device < 0 || device >= mfx_device_count()) {
    mfx_fail(device < 0 || device >= mfx_device_count() ? MFX_E_NODEVICE : MFX_E_INVAL,
             "mfx_seq_upload: bad argument (device %d of %d)", device, mfx_device_count());
    return nullptr;
  }
  DevGuard g(device);
  const double t_up0 = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
  mfx_seq *s = seq_layout(device, lens, ncontigs);
  const double t_up1 = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
  bool packed_transport = false;
  {
    const char *asc = getenv("MFX_UPLOAD_ASCII");
    const char *pm = getenv("MFX_UPLOAD_PACKED_MIN");          // bytes from which the packed transport pays (tests: 0)
    packed_transport = !(asc && atoi(asc)) && s->buf_bytes >= (pm ? strtoull(pm, nullptr, 10) : (uint64_t)(8u << 20));
  }
  if (seq_alloc(s, !packed_transport) != MFX_OK) { mfx_seq_free(s); return nullptr; }
  if (getenv("MFX_UPLOAD_TIMING"))
    fprintf(stderr, "-- upload: layout %.3f s, device buffers %.3f s\n", t_up1 - t_up0,
            std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() - t_up1);
  {
    // default: the sequence crosses the bus as its packed planes (0.375 B per base, encoded by the host threads); one byte per
    // base is made on the device when a kernel asks for it (mfx_seq_ensure_ascii).  MFX_UPLOAD_ASCII=1: the bytes themselves.
    if (packed_transport) {
      if (seq_upload_packed(s, bases) != MFX_OK) { mfx_seq_free(s); return nullptr; }
      return s;
    }
  }
  // The packed image (contigs at their padded offsets, zero filler in between) is assembled in a
  // pinned staging buffer and sent in large pieces: an assembly of a million small contigs must not
  // become a million tiny hipMemcpy calls.
  // Two staging buffers alternate: while one is in flight over PCIe the host fills the other.
  // (sized to the upload: pinning memory costs ~0.4 ms per MB, which a small upload should not pay 128 MB of)
  const size_t STAGE = (size_t)std::min<uint64_t>(64ull << 20, std::max<uint64_t>(1ull << 20, ((s->buf_bytes / 2 + (1ull << 20)) >> 20) << 20));
  uint8_t *stages[2] = {nullptr, nullptr};
  hipStream_t cs = nullptr;
  hipEvent_t done_ev[2] = {nullptr, nullptr};
  bool ok = hipHostMalloc((void **)&stages[0], STAGE, hipHostMallocDefault) == hipSuccess &&
            hipHostMalloc((void **)&stages[1], STAGE, hipHostMallocDefault) == hipSuccess &&
            hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&done_ev[0], hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&done_ev[1], hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    mfx_fail(MFX_E_NOMEM, "pinned staging setup failed");
    for (int i = 0; i < 2; ++i) { if (stages[i]) (void)hipHostFree(stages[i]); if (done_ev[i]) (void)hipEventDestroy(done_ev[i]); }
    if (cs) (void)hipStreamDestroy(cs);
    mfx_seq_free(s);
    return nullptr;
  }
  int cur = 0;
  bool inflight[2] = {false, false};
  uint8_t *stage = stages[0];
  uint64_t win = 0;                      // device offset the staging buffer currently mirrors
  size_t used = 0;                       // bytes of it that are meaningful
  auto flush = [&]() {
    if (used) {
      if (hipMemcpyAsync(s->d_bases + win, stage, used, hipMemcpyHostToDevice, cs) != hipSuccess ||
          hipEventRecord(done_ev[cur], cs) != hipSuccess) ok = false;
      inflight[cur] = true;
      cur ^= 1;
      if (inflight[cur] && hipEventSynchronize(done_ev[cur]) != hipSuccess) ok = false;   // the other buffer is free again
      inflight[cur] = false;
      stage = stages[cur];
    }
    win += used;
    used = 0;
  };
  for (uint32_t c = 0; c < ncontigs && ok; ++c) {
    uint64_t done = 0;
    while (done < lens[c] && ok) {
      const uint64_t dst = s->off[c] + done;                 // device offset of the next byte of this contig
      if (dst < win + used || dst - win >= STAGE) {          // not appendable to the current window
        flush();
        win = dst;
      }
      const size_t at = (size_t)(dst - win);
      if (at > used) memset(stage + used, 0, at - used);      // inter-contig padding stays non-ACGT
      const size_t m = (size_t)std::min<uint64_t>(lens[c] - done, STAGE - at);
      par_memcpy(stage + at, bases[c] + done, m);
      used = at + m;
      done += m;
      if (used == STAGE) flush();
    }
  }
  if (ok) flush();
  if (hipStreamSynchronize(cs) != hipSuccess) ok = false;
  for (int i = 0; i < 2; ++i) { (void)hipHostFree(stages[i]); (void)hipEventDestroy(done_ev[i]); }
  (void)hipStreamDestroy(cs);
  if (!ok) {
    mfx_fail(MFX_E_HIP, "H2D copy of the packed assembly failed");
    mfx_seq_free(s);
    return nullptr;
  }
  seq_pack_resident(s);
  return s;
}

extern "C" mfx_seq *mfx_seq_from_device(int device, const void *const *d_bases, const uint64_t *lens, uint32_t ncontigs,
                                        void *stream) {
  if ((ncontigs && (!d_bases || !lens)) || device < 0 || device >= mfx_device_count()) {
    mfx_fail(MFX_E_INVAL, "mfx_seq_from_device: bad argument");
    return nullptr;
  }
  DevGuard g(device);
  mfx_seq *s = seq_layout(device, lens, ncontigs);
  if (seq_alloc(s) != MFX_OK) { mfx_seq_free(s); return nullptr; }
  for (uint32_t c = 0; c < ncontigs; ++c)
    if (lens[c] && hipMemcpyAsync(s->d_bases + s->off[c], d_bases[c], lens[c], hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) {
      mfx_fail(MFX_E_HIP, "D2D copy of contig %u failed", c);
      mfx_seq_free(s);
      return nullptr;
    }
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {
    mfx_fail(MFX_E_HIP, "D2D copy sync failed");
    mfx_seq_free(s);
    return nullptr;
  }
  seq_pack_resident(s);
  return s;
}

extern "C" void mfx_seq_free(mfx_seq *s) {
  if (!s) return;
  DevGuard g(s->device);
  if (s->d_bases) (void)hipFree(s->d_bases);
  if (s->d_codes) (void)hipFree(s->d_codes);
  if (s->d_valid) (void)hipFree(s->d_valid);
  if (s->d_contig_off) (void)hipFree(s->d_contig_off);
  if (s->d_contig_len) (void)hipFree(s->d_contig_len);
  if (s->d_tile_start) (void)hipFree(s->d_tile_start);
  if (s->d_tile_contig) (void)hipFree(s->d_tile_contig);
  delete s;
}

extern "C" uint32_t mfx_seq_num_contigs(const mfx_seq *s) { return s ? s->ncontigs : 0; }
extern "C" uint64_t mfx_seq_num_bases(const mfx_seq *s) { return s ? s->total_bases : 0; }
extern "C" uint64_t mfx_seq_num_tiles(const mfx_seq *s) { return s ? s->ntiles : 0; }
extern "C" int mfx_seq_is_packed(const mfx_seq *s) { return s && (s->planes_ok || s->bases_stale) ? 1 : 0; }

// a sequence object without content: what a streamed run (mfx_stream.cpp) uploads into
extern "C" mfx_seq *mfx_seq_create(int device, const uint64_t *lens, uint32_t ncontigs) {
  if ((ncontigs && !lens) || device < 0 || device >= mfx_device_count()) {
    mfx_fail(device < 0 || device >= mfx_device_count() ? MFX_E_NODEVICE : MFX_E_INVAL,
             "mfx_seq_create: bad argument (device %d of %d)", device, mfx_device_count());
    return nullptr;
  }
  DevGuard g(device);
  mfx_seq *s = seq_layout(device, lens, ncontigs);
  if (seq_alloc(s, false) != MFX_OK) { mfx_seq_free(s); return nullptr; }      // what fills it decides which form it holds
  return s;
}

int seq_alloc_planes(mfx_seq *s) {
  if (s->d_codes) return MFX_OK;
  const uint64_t pw = seq_plane_words(s);
  MFX_HIP(hipMalloc((void **)&s->d_codes, pw * sizeof(uint64_t)));
  MFX_HIP(hipMalloc((void **)&s->d_valid, pw * sizeof(uint32_t)));
  MFX_HIP(mfx_memset_now(s->d_valid, 0, pw * sizeof(uint32_t)));           // no valid base behind the sequence
  MFX_HIP(mfx_memset_now(s->d_codes, 0, pw * sizeof(uint64_t)));
  return MFX_OK;
}

// the packed planes of a resident sequence (2-bit codes + one validity bit per base, the tile's own form), made on the device
extern "C" int mfx_seq_pack(mfx_seq *s) {
  if (!s) return mfx_fail(MFX_E_INVAL, "mfx_seq_pack: null argument");
  std::lock_guard<std::mutex> lazy(s->lazy_mu);
  if (s->planes_ok) return MFX_OK;
  DevGuard g(s->device);
  int rc = seq_alloc_planes(s);
  if (rc) return rc;
  if ((rc = seq_need_bases(s)) != MFX_OK) return rc;
  MFX_HIP(mfx_k_pack(s->d_bases, s->d_codes, s->d_valid, s->buf_bytes / 32, nullptr));
  MFX_HIP(hipDeviceSynchronize());
  s->planes_ok = true;
  return MFX_OK;
}

// host-side copy into the pinned staging buffer, split over a few threads for large pieces
// (a single thread moves ~12 GB/s, well under PCIe Gen5)
void par_memcpy(uint8_t *dst, const char *src, size_t n) {
  const unsigned nt = std::min<unsigned>(8u, std::max(1u, mfx_host_threads()));
  if (n < (8u << 20) || nt == 1) { memcpy(dst, src, n); return; }
  std::vector<std::thread> th;
  const size_t per = (n + nt - 1) / nt;
  for (unsigned t = 0; t < nt; ++t) {
    size_t b = std::min(n, t * per), e = std::min(n, b + per);
    if (e > b) th.emplace_back([=]() { memcpy(dst + b, src + b, e - b); });
  }
  for (auto &x : th) x.join();
}
