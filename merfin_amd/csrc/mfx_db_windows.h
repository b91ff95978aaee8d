// mfx_db_windows.h -- the window session of the sorted-database calls (mfx_db_merge.cpp, mfx_db_join.cpp, mfx_db_trio.cpp): N sorted flat
// databases are opened, key windows are planned over them (mfx_merge.h), each window's blocks are read and decoded on the device into one
// dense ascending run per input, the runs go to the call's kernel chain, and at the end the windows must have held what the headers say.
// A driver holds what is particular to its call: its arguments, its own buffers, its kernels, its result.
#pragma once
#include "mfx_db_internal.h"
#include "mfx_merge.h"
#include "mfx_join.h"
#include "mfx_spectrum.h"

#include <algorithm>
#include <initializer_list>
#include <memory>

#pragma GCC visibility push(hidden)

// ---- the inputs ---------------------------------------------------------------------------------------------------------------
struct MergeIn {                                               // one input: header, directory and escapes on the host, the blocks in the file
  std::string path;
  int fd = -1;
  FlatHeader h;
  std::vector<uint64_t> dir;
  uint64_t nblocks = 0;
  std::vector<uint64_t> ek;
  std::vector<uint32_t> ev;
  MergeIn() = default;
  MergeIn(const MergeIn &) = delete;
  MergeIn &operator=(const MergeIn &) = delete;
  ~MergeIn() { if (fd >= 0) close(fd); }
  uint64_t off(uint64_t b) const { return dir[2 * b + 1] & 0xffffffffffffull; }
};
typedef std::vector<std::unique_ptr<MergeIn>> MergeIns;

// header, directory and escape list of an input, by the loader's checks; every refusal names the file
int merge_open_input(const char *path, MergeIn &in, const char *who);
// `n` inputs opened behind those `ins` holds, one after the other: the null check, the refusal of k > 31 up front (wide: what the call says of
// its k-mers, as in "the sorted join takes"; nullptr: the call leaves such a file to merge_open_input), merge_open_input, then the input's k
// against that of ins[0] (one_k: how that refusal ends).  `who` begins every text.
int db_open_inputs(const char *const *paths, uint32_t n, const char *who, const char *wide, const char *one_k, MergeIns &ins);
// the first of ins[from ...] that `out_path` is (by device and inode: under another name too), -1: none, or no such file yet
int db_output_is_input(const char *out_path, const MergeIns &ins, size_t from = 0);

// ---- the windows, and a window's blocks decoded into one dense run per input -----------------------------------------------------
struct MergeWindows {                                          // the plan (mfx_merge.h) and what the largest window takes
  std::vector<mfx_merge_input> pin;
  std::vector<mfx_merge_window> win;
  std::vector<uint64_t> blk;
  uint64_t n_all = 0, max_pairs = 0, max_bytes = 0, max_tasks = 0, max_esc = 0;
};
int merge_plan_windows(const MergeIns &ins, int k, const char *who, MergeWindows &P);      // (MFX_MERGE_RANGE is read here)

struct MergeRun { uint64_t off, len; };
struct MergeDecoder {                                          // a window's way from the files to the runs, and the memory it goes through
  void *d_words = nullptr;                                     // max_bytes + 8: the window's blocks
  mfx_merge_task *d_tasks = nullptr;                           // max_tasks
  uint32_t *d_below = nullptr, *d_above = nullptr, *d_err = nullptr;      // max_tasks, max_tasks, one per input
  uint64_t *d_ek = nullptr;                                    // max_esc + 1: the window's escapes
  uint32_t *d_ev = nullptr;
  void *pinned = nullptr;                                      // max_bytes + 8 on the host: the blocks on their way to the device
  std::vector<mfx_merge_task> tasks;
  std::vector<uint64_t> hek, run_off, run_len, first_task;
  std::vector<uint32_t> hev, cnt, errs;
  std::vector<MergeRun> runs;                                  // per input: its dense run of the window in the decoded buffer
  double t_read = 0, t_decode = 0;                             // of the last window
  uint32_t zero_from = ~0u;                                    // mfx_db_merge_except: the inputs from this one on are subtracted
  MergeDecoder() = default;
  MergeDecoder(const MergeDecoder &) = delete;
  MergeDecoder &operator=(const MergeDecoder &) = delete;
  ~MergeDecoder() { if (pinned) (void)hipHostFree(pinned); }
  hipError_t init(const MergeWindows &P, uint32_t n_in);      // the buffers of the plan's largest window on the current device, and the pinned one
  uint64_t device_bytes() const { return bytes; }              // what init asks the device for
 private:
  DbDev dev;
  uint64_t bytes = 0;
};
// A call's device memory: the decoder's buffers, then sizes[i] bytes into own.p[i] (0: none).  hipSuccess, or what failed first; *total: the bytes
// of all of them, for the caller's text of what did not fit.
hipError_t db_alloc(MergeDecoder &dec, const MergeWindows &P, uint32_t n_in, DbDev &own, std::initializer_list<uint64_t> sizes, uint64_t *total);
// window wi: its blocks read (pread) and decoded on the device into keys / vals, D.runs the inputs' dense runs in them.  A block that decodes
// what no writer makes ends in MFX_E_FORMAT, naming the file.
int merge_decode_window(const MergeIns &ins, const MergeWindows &P, size_t wi, int k, const char *who, MergeDecoder &D, uint64_t *keys, uint32_t *vals);

// the pairwise merge tree over the runs in buffer `cur` of bk / bv, level by level from one buffer to the other: runs[0] is the merged run in
// the buffer `cur` names afterwards
int merge_tree(std::vector<MergeRun> &runs, uint64_t *const bk[2], uint32_t *const bv[2], int &cur);

// one pass over the windows: what it held of every input, how many windows had pairs, the time its reads and decodes took (added up over
// the passes of a call)
struct DbPass {
  std::vector<uint64_t> got;
  uint64_t windows = 0;
  double t_read = 0, t_decode = 0;
  explicit DbPass(size_t n_in) : got(n_in, 0) {}
  // what the windows held against what the files say: no partial result is handed out
  int check(const MergeIns &ins) const;
};
// every window that has pairs, decoded into keys / vals and handed to fn(runs): fn returns MFX_OK or what ends the call
template <class F>
int db_each_window(const MergeIns &ins, const MergeWindows &P, int k, const char *who, MergeDecoder &D, uint64_t *keys, uint32_t *vals, DbPass &pass, F &&fn) {
  std::fill(pass.got.begin(), pass.got.end(), 0);
  pass.windows = 0;
  for (size_t wi = 0; wi < P.win.size(); ++wi) {
    if (P.win[wi].pairs == 0) continue;
    const int rc_dec = merge_decode_window(ins, P, wi, k, who, D, keys, vals);
    pass.t_read += D.t_read; pass.t_decode += D.t_decode;
    if (rc_dec) return rc_dec;
    for (size_t i = 0; i < ins.size(); ++i) pass.got[i] += D.runs[i].len;
    ++pass.windows;
    if (int rc = fn(D.runs)) return rc;
  }
  return MFX_OK;
}

// ---- what the reductions at the end of a chain share -----------------------------------------------------------------------------
// the image's arguments as mfx_spectrum_run sets them; MFX_SPECTRUM_AGG is read here (docs/KNOBS.md)
mfx_spectrum_args db_spectrum_args(uint32_t copies, uint32_t max_mult, uint32_t lds_cols, uint64_t *img);
int db_upload_prob(const mfx_db_join_opts *o, uint32_t *d_K, double *d_P);      // the -prob table into o->n_prob entries each on the device
int db_grid(int device, int per_cu, int *grid);                // CUs x the workgroups a CU holds at once

#pragma GCC visibility pop
