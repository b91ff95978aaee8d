// mfx_histsum.h -- the layout of a -hist counts image on the HOST and the sum of several slots' images (host only, no HIP:
// tools/native/histsum_sanitize.cpp builds it with a plain C++ compiler).  An image is MFX_HIST_WORDS(nbins, ncontigs) words:
//   [0, nbins) undr bins | [nbins, 2 nbins) over bins | kasm | kmissing | novf | kasm per contig | kmissing per contig
// (novf: occurrences that fell into K* bins beyond the dense ones -- they wait in the evaluator's overflow list).  The kernels keep
// their own arithmetic for the same layout (mfx_device.h: c_glob).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/merfin_amd.h"

namespace mfx_histsum {
inline size_t undr(uint32_t) { return 0; }
inline size_t over(uint32_t nbins) { return nbins; }
inline size_t kasm(uint32_t nbins) { return 2ull * nbins + 0; }
inline size_t kmissing(uint32_t nbins) { return 2ull * nbins + 1; }
inline size_t novf(uint32_t nbins) { return 2ull * nbins + 2; }
inline size_t contig_kasm(uint32_t nbins) { return 2ull * nbins + 3; }
inline size_t contig_kmissing(uint32_t nbins, uint32_t ncontigs) { return contig_kasm(nbins) + ncontigs; }

// One slot's image `h` (ncontigs_slot contigs) added into the accumulator `acc` (ncontigs_total contigs): bins and the three global
// counters straight, the per-contig counters at contig_ids[i] (null: the slot's contigs ARE the accumulator's, in order).  Returns the
// slot's novf.  h == acc (a slot whose image is the accumulator) adds nothing.
inline uint64_t add(uint64_t *acc, uint32_t nbins, uint32_t ncontigs_total, const uint64_t *h, uint32_t ncontigs_slot, const uint32_t *contig_ids) {
  const uint64_t n = h[novf(nbins)];
  if (h == acc) return n;
  for (size_t i = 0; i < contig_kasm(nbins); ++i) acc[i] += h[i];
  for (uint32_t i = 0; i < ncontigs_slot; ++i) {
    const uint32_t c = contig_ids ? contig_ids[i] : i;
    acc[contig_kasm(nbins) + c] += h[contig_kasm(nbins) + i];
    acc[contig_kmissing(nbins, ncontigs_total) + c] += h[contig_kmissing(nbins, ncontigs_slot) + i];
  }
  return n;
}
}  // namespace mfx_histsum
