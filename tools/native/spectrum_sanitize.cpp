// Host side of the copy-number spectrum (csrc/mfx_spectrum.cpp: mfx_spectrum_peak, mfx_spectrum_write) under AddressSanitizer + UBSan,
// without a device: rows that are empty, hold one cell, hold only the overflow column, or hold UINT64_MAX everywhere (window sums beyond
// 64 bits), at the smallest and the largest max_mult; images of every `copies` through the plain and the compressed writer; arguments out
// of range.  Every call must return -- an error code where the input asks for one -- and the sanitizers must stay silent.
//   hipcc -fsanitize=address,undefined -g -O1 -std=c++17 tools/native/spectrum_sanitize.cpp merfin_amd/csrc/mfx_spectrum.cpp -Imerfin_amd/csrc -Iinclude \
//         -Lmerfin_amd -lmerfin_amd -Wl,-rpath,$PWD/merfin_amd -Wl,-rpath,/opt/rocm/lib -o /tmp/spectrum_sanitize && ASAN_OPTIONS=detect_leaks=0 /tmp/spectrum_sanitize /tmp
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "merfin_amd.h"

int main(int argc, char **argv) {
  const std::string dir = argc > 1 ? argv[1] : "/tmp";
  int bad = 0;
  auto expect = [&](const char *what, int rc, int want) {
    printf("%-52s rc=%d%s\n", what, rc, rc == want ? "" : "  <-- UNEXPECTED");
    bad += rc != want;
  };
  mfx_spectrum_peak_t pk;
  for (uint32_t mm : {4u, 5u, 6u, 50u, 65536u}) {
    std::vector<uint64_t> row(mm + 1, 0);                            // exactly max_mult + 1 cells: a read one past either end is caught
    char what[96];
    snprintf(what, sizeof what, "max_mult %u: empty row", mm);
    expect(what, mfx_spectrum_peak(row.data(), mm, &pk), MFX_E_NODATA);
    row[mm] = UINT64_MAX;
    snprintf(what, sizeof what, "max_mult %u: overflow column only", mm);
    expect(what, mfx_spectrum_peak(row.data(), mm, &pk), MFX_E_NODATA);
    row[mm] = 0;
    row[0] = UINT64_MAX;
    snprintf(what, sizeof what, "max_mult %u: column 0 only", mm);
    expect(what, mfx_spectrum_peak(row.data(), mm, &pk), MFX_E_NODATA);
    row[0] = 0;
    for (uint32_t at : {1u, 2u, mm / 2, mm - 2, mm - 1}) {
      row[at] = 1;
      const int rc = mfx_spectrum_peak(row.data(), mm, &pk);
      printf("max_mult %u: one cell at %u: rc=%d", mm, at, rc);
      if (rc == MFX_OK) printf(" (valley %u main %u haploid %u count %lu)", pk.valley, pk.main_peak, pk.haploid_peak, (unsigned long)pk.count_at_peak);
      printf("\n");
      bad += rc != MFX_OK && rc != MFX_E_NODATA;
      if (rc == MFX_OK) bad += pk.haploid_peak < 1 || pk.haploid_peak >= mm || pk.valley >= pk.main_peak;
      row[at] = 0;
    }
    std::vector<uint64_t> full(mm + 1, UINT64_MAX);
    const int rc = mfx_spectrum_peak(full.data(), mm, &pk);           // a flat row: valley 1, the first maximum beyond it
    printf("max_mult %u: UINT64_MAX everywhere: rc=%d (valley %u main %u haploid %u)\n", mm, rc, pk.valley, pk.main_peak, pk.haploid_peak);
    bad += rc != MFX_OK || pk.count_at_peak != UINT64_MAX;
    full[mm / 2] -= 1;
    bad += mfx_spectrum_peak(full.data(), mm, &pk) != MFX_OK;
  }
  std::vector<uint64_t> row(16, 1);
  expect("max_mult 3", mfx_spectrum_peak(row.data(), 3, &pk), MFX_E_INVAL);
  expect("max_mult 65537", mfx_spectrum_peak(row.data(), 65537, &pk), MFX_E_INVAL);
  expect("null row", mfx_spectrum_peak(nullptr, 10, &pk), MFX_E_INVAL);
  expect("null out", mfx_spectrum_peak(row.data(), 10, nullptr), MFX_E_INVAL);

  for (uint32_t copies = 1; copies <= 6; ++copies)
    for (uint32_t mm : {4u, 65536u})
      for (const char *suf : {".hist", ".hist.gz"}) {
        const size_t cells = (size_t)(copies + 2) * (mm + 1);
        for (int fill = 0; fill < 4; ++fill) {
          std::vector<uint64_t> img(cells, fill == 3 ? UINT64_MAX : 0);
          if (fill == 1) img[cells - 1] = 1;                           // one cell: the last of the last row
          if (fill == 2) for (uint32_t r = 0; r < copies + 2; ++r) img[(size_t)r * (mm + 1) + mm] = UINT64_MAX;      // all overflow
          if (fill == 3 && mm > 4) continue;                           // (a full 65537-column image is 8 MB of text per row: once is enough)
          const std::string p = dir + "/spectrum_sanitize" + suf;
          for (int ro = 0; ro < 2; ++ro) bad += mfx_spectrum_write(img.data(), copies, mm, ro, p.c_str()) != MFX_OK;
        }
      }
  printf("writer: every image of copies 1..6, max_mult 4 and 65536, plain and .gz written\n");
  expect("write: copies 0", mfx_spectrum_write(row.data(), 0, 4, 1, (dir + "/x").c_str()), MFX_E_INVAL);
  expect("write: copies 7", mfx_spectrum_write(row.data(), 7, 4, 1, (dir + "/x").c_str()), MFX_E_INVAL);
  expect("write: max_mult 3", mfx_spectrum_write(row.data(), 1, 3, 1, (dir + "/x").c_str()), MFX_E_INVAL);
  expect("write: null image", mfx_spectrum_write(nullptr, 1, 4, 1, (dir + "/x").c_str()), MFX_E_INVAL);
  expect("write: null path", mfx_spectrum_write(row.data(), 1, 4, 1, nullptr), MFX_E_INVAL);
  expect("write: a directory that is not there", mfx_spectrum_write(row.data(), 1, 4, 1, (dir + "/no/such/dir/x").c_str()), MFX_E_IO);
  printf(bad ? "FAILED: %d unexpected results\n" : "OK (%d unexpected results)\n", bad);
  return bad ? 1 : 0;
}
