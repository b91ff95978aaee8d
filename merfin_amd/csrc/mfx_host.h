// mfx_host.h -- what the host files of the library share besides mfx_internal.h: the scoped device helpers, the pieces of mfx_api.cpp,
// mfx_index.cpp, mfx_seq.cpp and mfx_dump.cpp that the other host files -- the several-slot drivers (mfx_multi.cpp), the transport of an
// assembly in host memory (mfx_stream.cpp), the variant modes' device calls (mfx_paths.cpp) -- are built from, and what mfx_multi.cpp and
// mfx_stream.cpp hand to each other.  Host only; no kernel file includes it.
#pragma once
#include "mfx_internal.h"
#include "mfx_kernels.h"

struct DevGuard {   // makes `dev` the current device for a scope
  int prev = -1;
  bool ok = false;
  explicit DevGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = (hipSetDevice(dev) == hipSuccess);
  }
  ~DevGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

template <class T>
struct DevBuf {   // scoped device scratch
  T *p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t n) { return hipMalloc((void **)&p, (n ? n : 1) * sizeof(T)); }
};

// the arguments of the lookup kernel (mfx_k_dump / mfx_kw_dump) over `npos` start positions from `src` (tile-aligned; the first `skip` are
// not written, `clen_left` bases of the contig remain from src), against ev's table and -prob table: -dump and the variant modes' lookups
static inline mfx_dump_args dump_args_of(const mfx_eval *ev, int canon, const uint8_t *src, uint64_t npos, uint64_t skip, uint64_t clen_left, uint32_t *readV,
                                         uint32_t *asmV, uint64_t *stats) {
  mfx_dump_args a;
  a.t = ev->ix->view();
  a.canonical = canon;
  a.src = src;
  a.npos = npos;
  a.skip = skip;
  a.clen_left = clen_left;
  a.readV = readV;
  a.asmV = asmV;
  a.peak = ev->peak;
  a.n_prob = ev->n_prob;
  a.probK = ev->d_probK;
  a.probP = ev->d_probP;
  a.stats = stats;
  return a;
}

// ---- defined in mfx_api.cpp ---------------------------------------------------
int index_canonical(const mfx_index *ix, int *canon);
int eval_run_resources(mfx_eval *ev, size_t words);      // the evaluator's counts image, its pinned mirror, d_kover and kernel streams (mfx_eval::sr), made once
int eval_run_enqueue(mfx_eval *ev, const mfx_seq *seq, uint32_t part_rank, uint32_t part_n);
int result_take_overflow(mfx_eval *ev, uint64_t novf, mfx_hist_result *out);
int ensure_tile_partials(mfx_eval *ev, uint64_t ntiles);
int hist_launch(mfx_eval *ev, const mfx_seq *seq, uint64_t tile_begin, uint64_t tile_end, uint32_t part_rank, uint32_t part_n, uint32_t part_shift,
                uint64_t *d_counts, double *d_kover, void *stream, uint64_t chunk_of_total = 0, int ctr_slot = 0, uint64_t partials_tile0 = 0);
hipError_t ovf_reset_hip(mfx_eval *ev, hipStream_t st);

// ---- defined in mfx_seq.cpp ---------------------------------------------------
void par_memcpy(uint8_t *dst, const char *src, size_t n);
int seq_need_bases(mfx_seq *s);          // d_bases allocated and cleared, if it is not there
void seq_digest_finish(const mfx_seq *s, uint64_t h);

// a sequence's packed planes: the words each holds (a tile reads 130 words from its first one), and their allocation
inline uint64_t seq_plane_words(const mfx_seq *s) { return s->buf_bytes / 32 + (MFX_TILE + 64) / 32 + 1; }
int seq_alloc_planes(mfx_seq *s);

// ---- defined in mfx_dump.cpp --------------------------------------------------
unsigned t_sharers_get();                // what the calling thread last passed to mfx_host_threads_share
// ---- defined in mfx_stream.cpp ------------------------------------------------
int seq_upload_packed(mfx_seq *seq, const char *const *bases);      // mfx_seq_upload's packed transport
// the streamed run over the tiles [tl, th) of an assembly in host memory (no part: all of them, and the result in `out`)
struct StreamPart {
  uint64_t tl = 0, th = 0;
  uint64_t *d_counts = nullptr;          // caller's device image / koverCpy to accumulate into (cleared by the caller); null: the evaluator's own, returned on the host
  double   *d_kover = nullptr;
  std::vector<double> *chunk_sums = nullptr;   // the first-level koverCpy sums of the part (4096 (tile, wave) values each), for a bit-stable sum over the parts
  bool      want_result = true;          // false: the image stays in ev->sr.h_img (or on the device), no mfx_hist_result is made
};
int hist_run_streamed_packed(mfx_eval *ev, mfx_seq *seq, const char *const *bases, mfx_hist_result *out, const StreamPart *part = nullptr);
