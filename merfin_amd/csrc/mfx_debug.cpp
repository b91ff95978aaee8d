// mfx_debug.cpp -- test-facing entries (include/merfin_amd.h: mfx_debug_*, mfx_eval_debug_worklist*; the -hist worklist's are at the end of
// the file).  Those over the variant modes' production functions: the suite
// otherwise sees the traverse and score kernels only through the selectors (bestFilter, bestVariant, ...), which reduce numM to a minimum
// and totdk to a truncated tie-break; these hand a caller the per-path values, the path text and the path table themselves.  Nothing here
// computes: the host entry runs mfx_traverse_cluster (the scalar instantiation of what the device's kernel runs per wave), the other two
// call mfx_score_paths / mfx_score_paths_trv.  What they add is the CHECK of the caller's tables: every offset a kernel would follow is
// inside its array before anything is launched.
#include "mfx_internal.h"
#include "mfx_kernels.h"

#include <stddef.h>
#include <string.h>

// the tables cross the C ABI as raw arrays (numpy structured dtypes in merfin_amd/binding.py): their layout is part of the ABI
static_assert(sizeof(mfx_trv_variant) == 16 && offsetof(mfx_trv_variant, off) == 0 && offsetof(mfx_trv_variant, reflen) == 4 &&
              offsetof(mfx_trv_variant, na) == 8 && offsetof(mfx_trv_variant, al0) == 12, "mfx_trv_variant: layout of the C ABI");
static_assert(sizeof(mfx_trv_allele) == 16 && offsetof(mfx_trv_allele, off) == 0 && offsetof(mfx_trv_allele, len) == 8 &&
              offsetof(mfx_trv_allele, pad) == 12, "mfx_trv_allele: layout of the C ABI");
static_assert(sizeof(mfx_trv_cluster) == 56 && offsetof(mfx_trv_cluster, win_off) == 0 && offsetof(mfx_trv_cluster, win_len) == 8 &&
              offsetof(mfx_trv_cluster, nv) == 12 && offsetof(mfx_trv_cluster, var0) == 16 && offsetof(mfx_trv_cluster, path_cap) == 20 &&
              offsetof(mfx_trv_cluster, text0) == 24 && offsetof(mfx_trv_cluster, path0) == 32 && offsetof(mfx_trv_cluster, row0) == 40 &&
              offsetof(mfx_trv_cluster, text_cap) == 48 && offsetof(mfx_trv_cluster, pad) == 52, "mfx_trv_cluster: layout of the C ABI");

namespace {

// every index of the cluster tables inside its array; the room of two clusters may not be told apart here (overlapping room is the caller's
// business: the kernels then write twice, inside the arrays)
int check_tables(const char *who, const mfx_trv_cluster *cl, uint64_t ncl, const mfx_trv_variant *var, uint64_t nvar, const mfx_trv_allele *al, uint64_t nal,
                 uint64_t win_bytes, uint64_t al_bytes, uint64_t text_begin, uint64_t text_end, uint64_t path_cap, uint64_t row_cap, bool every_slot) {
  // every_slot (the device call): the score kernel reads EVERY slot of the table, and a slot is written by the cluster it belongs to only
  std::vector<uint8_t> owned(every_slot ? path_cap : 0, 0);
  for (uint64_t c = 0; c < ncl; ++c) {
    const mfx_trv_cluster &C = cl[c];
    if (C.win_off > win_bytes || C.win_len > win_bytes - C.win_off) return mfx_fail(MFX_E_INVAL, "%s: cluster %lu: window outside the window text", who, (unsigned long)c);
    if (C.var0 > nvar || C.nv > nvar - C.var0) return mfx_fail(MFX_E_INVAL, "%s: cluster %lu: variants outside the table", who, (unsigned long)c);
    if (C.text0 < text_begin || C.text0 > text_end || C.text_cap > text_end - C.text0) return mfx_fail(MFX_E_INVAL, "%s: cluster %lu: text room outside [%lu, %lu)", who, (unsigned long)c, (unsigned long)text_begin, (unsigned long)text_end);
    if (C.path0 > path_cap || C.path_cap > path_cap - C.path0) return mfx_fail(MFX_E_INVAL, "%s: cluster %lu: path slots outside the table", who, (unsigned long)c);
    if (C.row0 > row_cap || (uint64_t)C.path_cap * C.nv > row_cap - C.row0) return mfx_fail(MFX_E_INVAL, "%s: cluster %lu: rows outside the table", who, (unsigned long)c);
    if (every_slot)
      for (uint64_t q = C.path0; q < C.path0 + C.path_cap; ++q) {
        if (owned[q]) return mfx_fail(MFX_E_INVAL, "%s: cluster %lu: path slot %lu belongs to an earlier cluster too", who, (unsigned long)c, (unsigned long)q);
        owned[q] = 1;
      }
    for (uint32_t i = 0; i < C.nv; ++i) {
      const mfx_trv_variant &V = var[C.var0 + i];
      if (V.al0 > nal || V.na > nal - V.al0) return mfx_fail(MFX_E_INVAL, "%s: cluster %lu, variant %u: alleles outside the table", who, (unsigned long)c, i);
      for (uint32_t j = 0; j < V.na; ++j) {
        const mfx_trv_allele &A = al[V.al0 + j];
        if (A.off > al_bytes || A.len > al_bytes - A.off) return mfx_fail(MFX_E_INVAL, "%s: cluster %lu, variant %u: allele %u outside the allele text", who, (unsigned long)c, i, j);
      }
    }
  }
  for (uint64_t q = 0; q < owned.size(); ++q)
    if (!owned[q]) return mfx_fail(MFX_E_INVAL, "%s: path slot %lu belongs to no cluster (nothing would write it before the score kernel reads it)", who, (unsigned long)q);
  return MFX_OK;
}

int check_paths(const char *who, uint64_t len, uint64_t npaths, uint64_t nvals, const uint64_t *off, const uint32_t *plen, const uint32_t *nv, const uint64_t *voff,
                const uint64_t *cfirst) {
  if (npaths && (!off || !plen || !nv || !voff || !cfirst)) return mfx_fail(MFX_E_INVAL, "%s: null argument", who);
  for (uint64_t p = 0; p < npaths; ++p) {
    if (off[p] > len || plen[p] > len - off[p]) return mfx_fail(MFX_E_INVAL, "%s: path %lu outside the text", who, (unsigned long)p);
    if (voff[p] > nvals || nv[p] > nvals - voff[p]) return mfx_fail(MFX_E_INVAL, "%s: path %lu: rows outside the table", who, (unsigned long)p);
    if (cfirst[p] > p) return mfx_fail(MFX_E_INVAL, "%s: path %lu: its cluster starts behind it", who, (unsigned long)p);
  }
  return MFX_OK;
}

}  // namespace

extern "C" int mfx_debug_traverse_host(const void *clusters, uint64_t ncl, const void *variants, uint64_t nvar, const void *alleles, uint64_t nal,
                                       const char *win_text, uint64_t win_bytes, const char *al_text, uint64_t al_bytes, uint64_t text_end, uint64_t path_cap,
                                       uint64_t row_cap, uint32_t *np, uint32_t *status, char *text, uint64_t *p_off, uint32_t *p_len, uint32_t *p_nv,
                                       uint64_t *p_voff, uint64_t *p_cfirst, int32_t *gt, uint32_t *vidx, uint32_t *vlen) {
  if ((ncl && (!clusters || !variants || !np || !status)) || (nal && !alleles) || (win_bytes && !win_text) || (al_bytes && !al_text) || (text_end && !text) ||
      (path_cap && (!p_off || !p_len || !p_nv || !p_voff || !p_cfirst)) || (row_cap && (!gt || !vidx || !vlen)))
    return mfx_fail(MFX_E_INVAL, "mfx_debug_traverse_host: null argument");
  const mfx_trv_cluster *cl = static_cast<const mfx_trv_cluster *>(clusters);
  const mfx_trv_variant *var = static_cast<const mfx_trv_variant *>(variants);
  const mfx_trv_allele *al = static_cast<const mfx_trv_allele *>(alleles);
  if (int rc = check_tables("mfx_debug_traverse_host", cl, ncl, var, nvar, al, nal, win_bytes, al_bytes, 0, text_end, path_cap, row_cap, false)) return rc;
  mfx_trv_out o;
  o.text = text;
  o.p_off = p_off; o.p_voff = p_voff; o.p_cfirst = p_cfirst; o.p_len = p_len; o.p_nv = p_nv;
  o.gt = gt; o.vidx = vidx; o.vlen = vlen;
  o.table_base = 0; o.row_base = 0;
  for (uint64_t c = 0; c < ncl; ++c) {
    status[c] = mfx_traverse_cluster(cl[c], var, al, win_text, al_text, o, &np[c]);
    for (uint64_t q = np[c]; q < cl[c].path_cap; ++q) {              // the slots not used, closed as mfx_var_traverse_kernel closes them
      const uint64_t e = cl[c].path0 + q;
      p_off[e] = cl[c].text0; p_len[e] = 0; p_nv[e] = 0; p_voff[e] = 0; p_cfirst[e] = e;
    }
  }
  return MFX_OK;
}

extern "C" int mfx_debug_score_paths(mfx_eval *ev, const char *text, uint64_t len, uint64_t npaths, uint64_t nvals, const uint64_t *off, const uint32_t *plen,
                                     const uint32_t *nv, const uint64_t *voff, const uint64_t *cfirst, const int32_t *gt, const uint32_t *vidx,
                                     const uint32_t *vlen, int need_dk, uint32_t *numM, double *totdk) {
  if (!ev || (nvals && (!gt || !vidx || !vlen))) return mfx_fail(MFX_E_INVAL, "mfx_debug_score_paths: null argument");
  if (int rc = check_paths("mfx_debug_score_paths", len, npaths, nvals, off, plen, nv, voff, cfirst)) return rc;
  mfx_path_table pt;
  pt.npaths = npaths; pt.nvals = nvals;
  pt.off = off; pt.len = plen; pt.nv = nv; pt.voff = voff; pt.cfirst = cfirst;
  pt.gt = gt; pt.vidx = vidx; pt.vlen = vlen;
  return mfx_score_paths(ev, text, len, &pt, need_dk, numM, totdk);
}

extern "C" int mfx_debug_score_paths_trv(mfx_eval *ev, const char *text, uint64_t len, uint64_t npaths, uint64_t nvals, const uint64_t *off, const uint32_t *plen,
                                         const uint32_t *nv, const uint64_t *voff, const uint64_t *cfirst, const int32_t *gt, const uint32_t *vidx,
                                         const uint32_t *vlen, const void *clusters, uint64_t ncl, const void *variants, uint64_t nvar, const void *alleles,
                                         uint64_t nal, const char *win_text, uint64_t win_bytes, const char *al_text, uint64_t al_bytes, uint64_t text_end,
                                         uint64_t path_cap, uint64_t row_cap, int need_dk, uint32_t *numM, double *totdk, uint32_t *np, uint32_t *status,
                                         char *text_out, uint64_t *p_off, uint32_t *p_len, uint32_t *p_nv, uint64_t *p_voff, uint64_t *p_cfirst, int32_t *gt_out,
                                         uint32_t *vidx_out, uint32_t *vlen_out) {
  if (!ev || (nvals && (!gt || !vidx || !vlen)) || (ncl && (!clusters || !variants || !np || !status)) || (nal && !alleles) || (win_bytes && !win_text) ||
      (al_bytes && !al_text) || !text_out || !p_off || !p_len || !p_nv || !p_voff || !p_cfirst || !gt_out || !vidx_out || !vlen_out)
    return mfx_fail(MFX_E_INVAL, "mfx_debug_score_paths_trv: null argument");
  if (text_end < len) return mfx_fail(MFX_E_INVAL, "mfx_debug_score_paths_trv: the device's room lies behind the host's text (text_end >= len)");
  if (int rc = check_paths("mfx_debug_score_paths_trv", len, npaths, nvals, off, plen, nv, voff, cfirst)) return rc;
  const mfx_trv_cluster *cl = static_cast<const mfx_trv_cluster *>(clusters);
  const mfx_trv_variant *var = static_cast<const mfx_trv_variant *>(variants);
  const mfx_trv_allele *al = static_cast<const mfx_trv_allele *>(alleles);
  if (int rc = check_tables("mfx_debug_score_paths_trv", cl, ncl, var, nvar, al, nal, win_bytes, al_bytes, len, text_end, path_cap, row_cap, true)) return rc;
  mfx_path_table pt;
  pt.npaths = npaths; pt.nvals = nvals;
  pt.off = off; pt.len = plen; pt.nv = nv; pt.voff = voff; pt.cfirst = cfirst;
  pt.gt = gt; pt.vidx = vidx; pt.vlen = vlen;
  mfx_trv_batch tb;
  tb.ncl = ncl; tb.nvar = nvar; tb.nal = nal; tb.win_bytes = win_bytes; tb.al_bytes = al_bytes;
  tb.cl = cl; tb.var = var; tb.al = al;
  tb.win_text = win_text; tb.al_text = al_text;
  tb.text_end = text_end; tb.path_cap = path_cap; tb.row_cap = row_cap;
  tb.np = np; tb.status = status; tb.p_len = p_len; tb.gt = gt_out;
  mfx_trv_readback rb;
  rb.text = text_out;
  rb.p_off = p_off; rb.p_voff = p_voff; rb.p_cfirst = p_cfirst; rb.p_nv = p_nv;
  rb.vidx = vidx_out; rb.vlen = vlen_out;
  return mfx_score_paths_trv(ev, text, len, &pt, &tb, need_dk, numM, totdk, &rb);
}

// ---------------------------------------------------------------------------
// The -hist worklist (mfx_hist_kernel's push_wave, mfx_hist_rest_kernel): how this evaluator's launches are given their list, and the
// list of the last launch read back.  hist_launch (mfx_api.cpp) applies the mode to every launch form; production never calls these.
// ---------------------------------------------------------------------------
extern "C" int mfx_eval_debug_worklist(mfx_eval *ev, int mode, uint32_t segcap) {
  if (!ev) return mfx_fail(MFX_E_INVAL, "mfx_eval_debug_worklist: null argument");
  if (mode < 0 || mode > 2) return mfx_fail(MFX_E_INVAL, "mfx_eval_debug_worklist: mode %d (0 no list, 1 default, 2 segments of at most segcap entries)", mode);
  if (mode == 2 && segcap == 0) return mfx_fail(MFX_E_INVAL, "mfx_eval_debug_worklist: mode 2 with segments of 0 entries (mode 0 turns the list off)");
  ev->dbg_wl_mode = mode;
  ev->dbg_wl_segcap = mode == 2 ? segcap : 0u;
  return MFX_OK;
}

extern "C" int mfx_eval_debug_worklist_read(mfx_eval *ev, int slot, uint32_t *segs, uint32_t *segcap, uint64_t *counts, uint64_t counts_cap, void *entries,
                                            uint64_t entries_cap, uint64_t *n_entries) {
  if (!ev || !segs || !segcap || !n_entries) return mfx_fail(MFX_E_INVAL, "mfx_eval_debug_worklist_read: null argument");
  if (slot < 0 || slot > 1) return mfx_fail(MFX_E_INVAL, "mfx_eval_debug_worklist_read: slot %d (0 or 1)", slot);
  *segs = ev->wl_used_segs[slot];
  *segcap = ev->wl_used_segcap[slot];
  *n_entries = 0;
  if (!*segs) return MFX_OK;                                   // the last launch of this slot had no list
  const uint64_t S = *segs, SC = *segcap;
  if (!ev->d_wl[slot] || S > MFX_WL_HEADER - 2 || S * SC > ev->wl_cap[slot])
    return mfx_fail(MFX_E_INVAL, "mfx_eval_debug_worklist_read: %lu segments of %lu entries do not lie in the list of %lu entries", (unsigned long)S,
                    (unsigned long)SC, (unsigned long)ev->wl_cap[slot]);
  int prev = 0;
  MFX_HIP(hipGetDevice(&prev));
  MFX_HIP(hipSetDevice(ev->device));
  struct Back { int d; ~Back() { (void)hipSetDevice(d); } } back{prev};
  MFX_HIP(hipDeviceSynchronize());
  std::vector<uint64_t> n(S);
  MFX_HIP(hipMemcpy(n.data(), ev->d_wl[slot] + 2, S * sizeof(uint64_t), hipMemcpyDeviceToHost));
  uint64_t total = 0;
  for (uint64_t g = 0; g < S; ++g) {
    if (n[g] > SC) return mfx_fail(MFX_E_INVAL, "mfx_eval_debug_worklist_read: segment %lu counts %lu entries, beyond its %lu", (unsigned long)g, (unsigned long)n[g], (unsigned long)SC);
    total += n[g];
  }
  *n_entries = total;
  if (counts) {
    if (counts_cap < S) return mfx_fail(MFX_E_INVAL, "mfx_eval_debug_worklist_read: %lu segments, the caller's counts hold %lu", (unsigned long)S, (unsigned long)counts_cap);
    memcpy(counts, n.data(), S * sizeof(uint64_t));
  }
  if (entries) {                                               // segment after segment, each with its own count of 16-byte records
    if (entries_cap < total) return mfx_fail(MFX_E_INVAL, "mfx_eval_debug_worklist_read: %lu entries, the caller's buffer holds %lu", (unsigned long)total, (unsigned long)entries_cap);
    uint8_t *dst = static_cast<uint8_t *>(entries);
    for (uint64_t g = 0; g < S; ++g) {
      if (n[g]) MFX_HIP(hipMemcpy(dst, ev->d_wl[slot] + MFX_WL_HEADER + 2 * g * SC, n[g] * 16, hipMemcpyDeviceToHost));
      dst += n[g] * 16;
    }
  }
  return MFX_OK;
}
