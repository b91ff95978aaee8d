// mfx_db_internal.h -- what the files of the k-mer database code share.  The definitions are mfx_db.cpp's (formats, converter, writer, index
// image); the window session (mfx_db_windows.h) and the drivers of the sorted-database calls (mfx_db_merge.cpp, mfx_db_join.cpp,
// mfx_db_trio.cpp) use them.  Nothing here is part of the library's ABI.
#pragma once
#include "mfx_internal.h"
#include "mfx_kernels.h"

#include <unistd.h>

#include <chrono>
#include <exception>
#include <new>
#include <string>
#include <vector>

// the writer that takes several tables (mfx_db_writer_*): the host arrays of the database so far, ascending
struct mfx_db_writer {
  std::string path;
  int k = 0;
  std::vector<uint64_t> keys;
  std::vector<uint32_t> vals;
  // the streamed kind (mfx_db_writer_open_streamed): the blocks go to the spool <path>.blocks as they are made.  What stays on the host is
  // the directory (16 bytes per MFX_DELTA_BLOCK k-mers), the escapes and the carry: the fewer than MFX_DELTA_BLOCK pairs behind the last
  // full block.  close writes header and directory, puts the spool behind them, then the escapes: the bytes of write_flat_delta.
  bool streamed = false;
  std::string spool;
  int fd = -1;
  uint64_t n = 0, spool_bytes = 0;                             // k-mers appended (those of the carry too); bytes of the spool
  std::vector<uint64_t> dir;                                   // per block written: its first k-mer, its spool offset | kb << 48 | vb << 56
  std::vector<uint64_t> ek;                                    // the escapes, in the file's order
  std::vector<uint32_t> ev;
  std::vector<uint64_t> ck;                                    // the carry
  std::vector<uint32_t> cv;
  uint64_t last = 0;                                           // the last k-mer appended (n > 0)
  size_t bounce = 16u << 20;                                   // bytes of one pinned bounce buffer (MFX_DB_BOUNCE, read at open)
  double t_export = 0, t_sort = 0, t_plan = 0, t_pack = 0, t_copy = 0, t_spool = 0;      // MFX_DB_TIMING
  bool merging = false;                                        // mfx_db_merge's writer: its split has these in the place of export and sort
  double t_read = 0, t_decode = 0, t_merge = 0, t_combine = 0;
  ~mfx_db_writer() {
    if (fd >= 0) close(fd);
    if (streamed && !spool.empty()) unlink(spool.c_str());
  }
};

#pragma GCC visibility push(hidden)

// ---- the flat binary file (the payloads: mfx_db.cpp) -----------------------------------------------------------------------
struct FlatHeader {
  char     magic[8];     // "MFXKMER1"
  uint32_t k;
  uint32_t flags;        // bit 0: canonical; bit 1: PACKED records (k <= 21); bit 2: DELTA-coded blocks (sorted k-mers, k <= 31)
  uint64_t n;
  uint64_t n_escape;     // packed: records whose count did not fit the record (was: reserved, 0)
};
constexpr uint32_t FLAT_PACKED = 2u;
constexpr uint32_t FLAT_DELTA = 4u;
constexpr uint32_t FLAT_PLACED = 8u;                           // (bits 8-15 of `flags`: MFX_PLACE_VERSION of the functions that made P)

const char *flat_header_problem(const FlatHeader &h, uint64_t fsize);      // nullptr = acceptable, else what is wrong
// a k-mer of k <= 31 bases has no bit at or above 2k
inline bool flat_key_fits(uint64_t key, uint32_t k) { return k >= 32 || (key >> (2 * k)) == 0; }
int read_delta_directory(int fd, const char *path, const FlatHeader &h, uint64_t fsize, std::vector<uint64_t> &dir, uint64_t *nblocks_out,
                         uint64_t *expect_out);
int detect(const std::string &path);                           // MFX_DB_FLAT, _TEXT, _MERYL; 0: no such file
int mfx_db_probe_impl(const char *path, mfx_db_info *out);

// ---- small helpers ----------------------------------------------------------------------------------------------------------
struct DbDev {                                                 // device buffers of one call, freed on every way out
  void *p[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  ~DbDev() { for (void *x : p) if (x) (void)hipFree(x); }
};
struct DeviceBack {                                            // the caller's device again on every way out
  int d = -1;
  DeviceBack() { if (hipGetDevice(&d) != hipSuccess) d = -1; }
  ~DeviceBack() { if (d >= 0) (void)hipSetDevice(d); }
};
// the body of an extern "C" entry: nothing leaves the C ABI as an exception
template <class F>
int db_guard(const char *who, F &&fn) {
  try { return fn(); }
  catch (const std::bad_alloc &) { return mfx_fail(MFX_E_NOMEM, "%s: out of memory", who); }
  catch (const std::exception &e) { return mfx_fail(MFX_E_IO, "%s: %s", who, e.what()); }
}
inline double db_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ---- the streamed writer, fed from the device ---------------------------------------------------------------------------------
struct WriterAbort {                                           // the writer of a call that does not reach close: the spool goes with it
  mfx_db_writer *w = nullptr;
  ~WriterAbort() { if (w) mfx_db_writer_abort(w); }
};
struct DbBounce {                                              // two pinned buffers and their events: the packed bytes' way to the spool
  void *pin[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~DbBounce() {
    for (void *x : pin) if (x) (void)hipHostFree(x);
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  }
};
// what stream_append_device needs beside the pairs, for appends of at most `cap` pairs (the carry in front of them counted): plan and offsets
// of the blocks on the device and on the host, the escapes' buffers (grown to what an append escapes), the bounce buffers
struct StreamDev {
  DbDev D;                                                     // p[0]: plan and offsets of the blocks; p[1], p[2]: the escapes' k-mers and counts
  DbBounce B;
  uint64_t cap = 0, maxb = 0, esc_cap = 0;
  std::vector<mfx_delta_plan> plan;
  std::vector<uint64_t> woff;
  std::vector<uint32_t> eoff;
};
int db_open_streamed(const char *path, int k, mfx_db_writer **out);
int stream_dev_init(StreamDev &S, const mfx_db_writer *w, uint64_t cap, const char *who, const char *knob);
int stream_append_device(mfx_db_writer *w, StreamDev &S, uint64_t *s_keys, uint32_t *s_vals, uint64_t rn, uint64_t *d_out, uint64_t out_bytes,
                         const char *who, const char *knob);

#pragma GCC visibility pop
