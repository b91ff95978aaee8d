// mfx_paths.cpp -- the device calls of the variant modes: a batch of paths looked up and scored (mfx_score_paths, mfx_score_paths_trv),
// a batch claimed into the path-only index (mfx_claim_paths_*).  Every array of a call is a piece of ONE allocation (mfx_var_arena.h) that
// its owner -- the evaluator, the claiming caller -- keeps from batch to batch: a run scores ~40 batches of the same size, and ~20
// allocations and as many frees per batch, each a device-wide wait, were a third of a batch's 7 ms.
#include "mfx_host.h"
#include "mfx_kernels.h"
#include "mfx_var_arena.h"

#include <algorithm>
#include <mutex>

static_assert(MFX_VAR_TILE == MFX_TILE, "mfx_var_arena.h: the text piece is sized in tiles");

// the owner's allocation made to hold `need` bytes (and a quarter more, if it has to be made again)
static int grow(uint8_t **buf, uint64_t *have, uint64_t need, const char *who) {
  if (need <= *have) return MFX_OK;
  if (*buf) { (void)hipFree(*buf); *buf = nullptr; *have = 0; }
  const uint64_t want = need + need / 4;
  if (hipMalloc((void **)buf, want) != hipSuccess) { (void)hipGetLastError(); *buf = nullptr; return mfx_fail(MFX_E_NOMEM, "%s: no device memory for a batch of paths (%.1f GB)", who, want / 1e9); }
  *have = want;
  return MFX_OK;
}

// the batch's text on the device: the host's paths copied in, the rest '\n' (no k-mer) until the traverse kernel writes its paths; the
// tile loads of the lookup and claim kernels reach a tile past the end
static int put_text(const mfx_var_arena &A, const char *text, uint64_t len, hipStream_t st) {
  MFX_HIP(mfx_memset_now(A.text + len, '\n', A.text_bytes - len));
  if (len) MFX_HIP(hipMemcpyAsync(A.text, text, len, hipMemcpyHostToDevice, st));
  return MFX_OK;
}

// the device part's tables go up and its clusters are enumerated: their paths into the text, their entries of the path table from slot
// table_base / row row_base on
static int traverse(const mfx_var_arena &A, const mfx_trv_batch *tb, uint64_t table_base, uint64_t row_base, hipStream_t st) {
  MFX_HIP(hipMemcpyAsync(A.cl, tb->cl, tb->ncl * sizeof(mfx_trv_cluster), hipMemcpyHostToDevice, st));
  MFX_HIP(hipMemcpyAsync(A.var, tb->var, tb->nvar * sizeof(mfx_trv_variant), hipMemcpyHostToDevice, st));
  if (tb->nal) MFX_HIP(hipMemcpyAsync(A.al, tb->al, tb->nal * sizeof(mfx_trv_allele), hipMemcpyHostToDevice, st));
  if (tb->win_bytes) MFX_HIP(hipMemcpyAsync(A.win, tb->win_text, tb->win_bytes, hipMemcpyHostToDevice, st));
  if (tb->al_bytes) MFX_HIP(hipMemcpyAsync(A.alt, tb->al_text, tb->al_bytes, hipMemcpyHostToDevice, st));
  mfx_trv_out o;
  o.text = reinterpret_cast<char *>(A.text);
  o.p_off = A.off + table_base; o.p_voff = A.voff + table_base; o.p_cfirst = A.cfirst + table_base; o.p_len = A.len + table_base; o.p_nv = A.nv + table_base;
  o.gt = A.gt + row_base; o.vidx = A.vidx + row_base; o.vlen = A.vlen + row_base;
  o.table_base = table_base; o.row_base = row_base;
  MFX_HIP(mfx_k_var_traverse(A.cl, tb->ncl, A.var, A.al, A.win, A.alt, o, A.np, A.status, st));
  return MFX_OK;
}

// What both scoring calls do once their arguments are accepted and the index's `canon` is known: the host's paths (text, pt) and the
// device part (tb; empty: none) become one text and one path table in the evaluator's arena, one lookup and one scoring launch run over them.
static int score_batch(mfx_eval *ev, int canon, const char *text, uint64_t len, const mfx_path_table *pt, const mfx_trv_batch *tb, int need_dk, uint32_t *numM,
                       double *totdk, const mfx_trv_readback *rb) {
  const uint64_t hp = pt->npaths, hv = pt->nvals, NP = hp + tb->path_cap;
  mfx_var_sizes z;
  z.total = std::max<uint64_t>(tb->text_end, len);
  z.npaths = NP; z.nvals = hv + tb->row_cap;
  z.ncl = tb->ncl; z.nvar = tb->nvar; z.nal = tb->nal; z.win_bytes = tb->win_bytes; z.al_bytes = tb->al_bytes;
  z.need_dk = need_dk != 0;
  std::lock_guard<std::mutex> scratch_lock(ev->var_scratch_mu);
  if (int rc = grow(&ev->d_var_scratch, &ev->var_scratch_bytes, mfx_var_arena_lay(z, nullptr, nullptr), "mfx_score_paths")) return rc;
  mfx_var_arena A;
  mfx_var_arena_lay(z, ev->d_var_scratch, &A);
  hipStream_t st = nullptr;
  if (int rc = put_text(A, text, len, st)) return rc;
  MFX_HIP(hipMemsetAsync(A.stats, 0, 2 * sizeof(uint64_t), st));
  if (hp) {
    MFX_HIP(hipMemcpyAsync(A.off, pt->off, hp * 8, hipMemcpyHostToDevice, st));
    MFX_HIP(hipMemcpyAsync(A.len, pt->len, hp * 4, hipMemcpyHostToDevice, st));
    MFX_HIP(hipMemcpyAsync(A.nv, pt->nv, hp * 4, hipMemcpyHostToDevice, st));
    MFX_HIP(hipMemcpyAsync(A.voff, pt->voff, hp * 8, hipMemcpyHostToDevice, st));
    MFX_HIP(hipMemcpyAsync(A.cfirst, pt->cfirst, hp * 8, hipMemcpyHostToDevice, st));
  }
  if (hv) {
    MFX_HIP(hipMemcpyAsync(A.gt, pt->gt, hv * 4, hipMemcpyHostToDevice, st));
    MFX_HIP(hipMemcpyAsync(A.vidx, pt->vidx, hv * 4, hipMemcpyHostToDevice, st));
    MFX_HIP(hipMemcpyAsync(A.vlen, pt->vlen, hv * 4, hipMemcpyHostToDevice, st));
  }
  if (tb->ncl)
    if (int rc = traverse(A, tb, hp, hv, st)) return rc;
  const mfx_dump_args a = dump_args_of(ev, canon, A.text, z.total, 0, z.total, A.readV, A.asmV, A.stats);
  MFX_HIP(ev->ix->wide() ? mfx_kw_dump(a, st) : mfx_k_dump(a, st));
  mfx_var_score_args sa;
  sa.text = A.text;
  sa.readV = A.readV; sa.asmV = A.asmV;
  sa.npaths = NP;
  sa.off = A.off; sa.len = A.len; sa.nv = A.nv; sa.voff = A.voff; sa.cfirst = A.cfirst;
  sa.gt = A.gt; sa.vidx = A.vidx; sa.vlen = A.vlen;
  sa.k = (uint32_t)ev->ix->k;
  sa.need_dk = need_dk ? 1 : 0;
  sa.peak = ev->peak; sa.n_prob = ev->n_prob; sa.probK = ev->d_probK; sa.probP = ev->d_probP;
  sa.numM = A.numM; sa.totdk = A.totdk;
  MFX_HIP(mfx_k_var_score(sa, st));
  MFX_HIP(hipMemcpy(numM, A.numM, NP * 4, hipMemcpyDeviceToHost));
  if (need_dk) MFX_HIP(hipMemcpy(totdk, A.totdk, NP * 8, hipMemcpyDeviceToHost));
  if (tb->ncl) {
    MFX_HIP(hipMemcpy(tb->np, A.np, tb->ncl * 4, hipMemcpyDeviceToHost));
    MFX_HIP(hipMemcpy(tb->status, A.status, tb->ncl * 4, hipMemcpyDeviceToHost));
    if (tb->path_cap) MFX_HIP(hipMemcpy(tb->p_len, A.len + hp, tb->path_cap * 4, hipMemcpyDeviceToHost));
    if (tb->row_cap) MFX_HIP(hipMemcpy(tb->gt, A.gt + hv, tb->row_cap * 4, hipMemcpyDeviceToHost));
  }
  if (rb) {
    MFX_HIP(hipMemcpy(rb->text, A.text, z.total, hipMemcpyDeviceToHost));
    if (tb->path_cap) {
      MFX_HIP(hipMemcpy(rb->p_off, A.off + hp, tb->path_cap * 8, hipMemcpyDeviceToHost));
      MFX_HIP(hipMemcpy(rb->p_voff, A.voff + hp, tb->path_cap * 8, hipMemcpyDeviceToHost));
      MFX_HIP(hipMemcpy(rb->p_cfirst, A.cfirst + hp, tb->path_cap * 8, hipMemcpyDeviceToHost));
      MFX_HIP(hipMemcpy(rb->p_nv, A.nv + hp, tb->path_cap * 4, hipMemcpyDeviceToHost));
    }
    if (tb->row_cap) {
      MFX_HIP(hipMemcpy(rb->vidx, A.vidx + hv, tb->row_cap * 4, hipMemcpyDeviceToHost));
      MFX_HIP(hipMemcpy(rb->vlen, A.vlen + hv, tb->row_cap * 4, hipMemcpyDeviceToHost));
    }
  }
  return MFX_OK;
}

static const char *const SEQ_ONLY_REFUSAL = "mfx_score_paths: a sequence-only index holds the k-mers of one sequence; alternative paths need the full index (or the path-only one: mfx_index_claim_paths)";

int mfx_score_paths(mfx_eval *ev, const char *text, uint64_t len, const mfx_path_table *pt, int need_dk, uint32_t *numM, double *totdk) {
  if (!ev || !pt || (len && !text) || (pt->npaths && (!numM || !pt->cfirst || (need_dk && !totdk)))) return mfx_fail(MFX_E_INVAL, "mfx_score_paths: null argument");
  if (pt->npaths == 0 || len == 0) return MFX_OK;
  DevGuard g(ev->device);
  int canon = 0;
  int rc = index_canonical(ev->ix, &canon);
  if (rc) return rc;
  if (ev->ix->seq_only && !ev->ix->paths_token) return mfx_fail(MFX_E_INVAL, "%s", SEQ_ONLY_REFUSAL);
  static const mfx_trv_batch no_device_part;
  return score_batch(ev, canon, text, len, pt, &no_device_part, need_dk, numM, totdk, nullptr);
}

int mfx_score_paths_trv(mfx_eval *ev, const char *text, uint64_t len, const mfx_path_table *pt, const mfx_trv_batch *tb, int need_dk, uint32_t *numM, double *totdk,
                        const mfx_trv_readback *rb) {
  if (!ev || !pt || !tb || (len && !text) || !numM || (need_dk && !totdk) || (tb->ncl && (!tb->cl || !tb->var || !tb->al || !tb->np || !tb->status || !tb->p_len || !tb->gt)))
    return mfx_fail(MFX_E_INVAL, "mfx_score_paths_trv: null argument");
  if (ev->ix->seq_only && !ev->ix->paths_token) return mfx_fail(MFX_E_INVAL, "%s", SEQ_ONLY_REFUSAL);
  if (pt->npaths + tb->path_cap == 0 || std::max<uint64_t>(tb->text_end, len) == 0) return MFX_OK;
  DevGuard g(ev->device);
  int canon = 0;
  int rc = index_canonical(ev->ix, &canon);
  if (rc) return rc;
  return score_batch(ev, canon, text, len, pt, tb, need_dk, numM, totdk, rb);
}

int mfx_claim_paths_batch(mfx_index *ix, uint8_t **scratch, uint64_t *scratch_bytes, const char *text, uint64_t len, const mfx_trv_batch *tb, uint64_t *bad) {
  if (!ix || !scratch || !scratch_bytes || (len && !text) || (tb && tb->ncl && (!tb->cl || !tb->var || !tb->al || !tb->status)))
    return mfx_fail(MFX_E_INVAL, "mfx_index_claim_paths: null argument");
  if (!ix->seq_only || ix->wide()) return mfx_fail(MFX_E_INVAL, "mfx_index_claim_paths: not a sequence-only index of k <= %d (mfx_index_create_for_seq)", MFX_MAX_K_NARROW);
  if (ix->frozen) return mfx_fail(MFX_E_INVAL, "mfx_index_claim_paths: this index already took counts; its k-mers must all be claimed before the first add / load");
  if (bad) *bad = 0;
  const uint64_t ncl = tb ? tb->ncl : 0;
  mfx_var_sizes z;
  z.claim = true;
  z.total = std::max<uint64_t>(tb ? tb->text_end : 0, len);
  if (tb) { z.npaths = tb->path_cap; z.nvals = tb->row_cap; z.ncl = ncl; z.nvar = tb->nvar; z.nal = tb->nal; z.win_bytes = tb->win_bytes; z.al_bytes = tb->al_bytes; }
  if (z.total == 0) return MFX_OK;
  DevGuard g(ix->device);
  if (int rc = grow(scratch, scratch_bytes, mfx_var_arena_lay(z, nullptr, nullptr), "mfx_index_claim_paths")) return rc;
  mfx_var_arena A;
  mfx_var_arena_lay(z, *scratch, &A);
  hipStream_t st = nullptr;
  if (int rc = put_text(A, text, len, st)) return rc;
  const uint64_t ntiles = (z.total + MFX_TILE - 1) / MFX_TILE;
  const uint64_t geo[4] = {0, z.total, 0, ntiles};                      // contig_off[1], contig_len[1], tile_start[2] of the one contig the text is
  MFX_HIP(hipMemcpyAsync(A.geo, geo, sizeof(geo), hipMemcpyHostToDevice, st));
  if (ncl)
    if (int rc = traverse(A, tb, 0, 0, st)) return rc;
  mfx_count_args a;
  a.t = ix->view();
  a.bases = A.text;
  a.contig_off = A.geo; a.contig_len = A.geo + 1; a.tile_start = A.geo + 2;
  a.ncontigs = 1;
  a.ntiles = ntiles;
  a.meta = ix->d_meta;
  a.count = 0;
  MFX_HIP(mfx_k_count(a, st));
  if (ncl) {
    MFX_HIP(hipMemcpy(tb->status, A.status, ncl * 4, hipMemcpyDeviceToHost));
    uint64_t nb = 0;
    for (uint64_t c = 0; c < ncl; ++c) nb += tb->status[c] != MFX_TRV_OK;
    if (bad) *bad = nb;
  } else MFX_HIP(hipStreamSynchronize(st));                             // (the host's text may go once this returns)
  return MFX_OK;
}
int mfx_claim_paths_finish(mfx_index *ix, uint64_t token) {
  if (!ix) return mfx_fail(MFX_E_INVAL, "mfx_index_claim_paths: null argument");
  DevGuard g(ix->device);
  MFX_HIP(hipDeviceSynchronize());
  if (int rc = mfx_index_check(ix)) return rc;
  ix->paths_token = token ? token : 1;
  ix->seq_digest = (uint32_t)(token >> 32) | 0x80000000u;              // (no sequence's k-mers: -hist / -dump of a sequence on this index are refused, mfx_check_seq_of_index)
  return MFX_OK;
}
void mfx_claim_paths_release(int device, uint8_t *scratch) {
  if (!scratch) return;
  DevGuard g(device);
  (void)hipFree(scratch);
}
