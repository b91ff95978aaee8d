// merfin (MI355X) -- command-line driver with the flag surface of the reference
// driver (src/merfin/merfin.C:79-155, validation :159-181) on top of the
// merfin_amd C ABI.  The pthread sweatShop pipeline (merfin.C:366-414) is
// replaced by: read all contigs -> pack into HBM -> one kernel launch per mode.
//
// Report types: -hist, -dump, -completeness, and the variant modes -filter /
// -polish / -better / -strict / -loose (paths enumerated on the host, every
// path k-mer scored on the GPU).
#include <libgen.h>
#include <math.h>
#include <dirent.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <unistd.h>
#include <future>
#include <thread>
#include <memory>
#include <string>
#include <vector>

#include "args.h"                 // Globals, the flags' parser and checks
#include "fasta.h"
#include "../csrc/mfx_grow.h"     // mfx_cut_bins: the key ranges of -count -passes

// load_Kmetric, merfin-globals.C:21-62
static bool load_Kmetric(Globals &G) {
  if (!G.pLookupTable) return true;
  fprintf(stderr, "-- Loading probability table '%s'.\n\n", G.pLookupTable);
  // compressedFileReader (merfin-globals.C:34): a table named *.gz / *.bz2 / *.xz is read through its decompressor
  mfx_file pf = mfx_open_reader(G.pLookupTable);
  FILE *f = pf.f;
  if (!f) {
    fprintf(stderr, "ERROR: Probability table (-prob) file '%s' doesn't exist!\n", G.pLookupTable);
    return false;
  }
  char line[4096];
  unsigned lineNum = 0;
  while (fgets(line, sizeof(line), f)) {
    size_t L = strlen(line);
    while (L && (line[L - 1] == '\n' || line[L - 1] == '\r')) line[--L] = 0;
    std::string keep(line);
    std::vector<char *> w;
    for (char *s = line; *s;) {
      while (*s == ',') *s++ = 0;
      if (!*s) break;
      w.push_back(s);
      while (*s && *s != ',') ++s;
    }
    if (w.size() == 2) {
      unsigned k = (unsigned)strtoul(w[0], nullptr, 10);
      double p = strtod(w[1], nullptr);
      G.copyKmerK.push_back(k);
      G.copyKmerP.push_back(p);
      lineNum++;
      fprintf(stderr, "Copy-number: %u\t\tReadK: %u\tProbability: %f\n", lineNum, k, p);
    } else {
      fprintf(stderr, "Copy-number: invalid line %u:  '%s'\n", lineNum, keep.c_str());
    }
  }
  if (mfx_close(pf) != 0) {
    fprintf(stderr, "ERROR: reading the probability table (-prob) '%s' failed (decompressor or read error).\n", G.pLookupTable);
    return false;
  }
  return true;
}

// Digest of what an index image was built from: every input's path, size and modification time (for a meryl
// directory: of each file in it) plus -min/-max.  A changed assembly -- the iterative polish workflow -- or a
// changed filter gives another digest, and the cached image is rebuilt instead of silently reused.
static void fp_mix(uint64_t &h, const void *p, size_t n) {
  const unsigned char *b = (const unsigned char *)p;
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 0x100000001b3ULL; }       // FNV-1a
}
static void fp_path(uint64_t &h, const char *path) {
  if (!path) { fp_mix(h, "-", 1); return; }
  fp_mix(h, path, strlen(path) + 1);
  struct stat st;
  if (stat(path, &st) != 0) return;
  if (S_ISDIR(st.st_mode)) {
    std::vector<std::string> names;
    if (DIR *d = opendir(path)) {
      while (struct dirent *e = readdir(d)) if (e->d_name[0] != '.') names.push_back(e->d_name);
      closedir(d);
    }
    std::sort(names.begin(), names.end());
    for (auto &n : names) {
      std::string f = std::string(path) + "/" + n;
      struct stat fs;
      if (stat(f.c_str(), &fs) != 0) continue;
      fp_mix(h, n.c_str(), n.size() + 1);
      uint64_t v[3] = {(uint64_t)fs.st_size, (uint64_t)fs.st_mtim.tv_sec, (uint64_t)fs.st_mtim.tv_nsec};
      fp_mix(h, v, sizeof(v));
    }
  } else {
    uint64_t v[3] = {(uint64_t)st.st_size, (uint64_t)st.st_mtim.tv_sec, (uint64_t)st.st_mtim.tv_nsec};
    fp_mix(h, v, sizeof(v));
  }
}
static uint64_t input_fingerprint(const Globals &G, bool seqOnly) {
  uint64_t h = 0xcbf29ce484222325ULL;
  fp_path(h, G.readDBname);
  for (const char *r : G.readsNames) fp_path(h, r);
  if (!G.readsNames.empty()) { const uint64_t kk = (uint64_t)G.kArg; fp_mix(h, &kk, sizeof(kk)); fp_mix(h, "reads", 6); }
  fp_path(h, G.seqDBname);
  if (!G.seqDBname || seqOnly) fp_path(h, G.seqName);   // the assembly side is counted from -sequence / the table holds ITS k-mers only
  if (seqOnly) fp_mix(h, "seq-only", 9);
  uint64_t v[2] = {G.minV, G.maxV};
  fp_mix(h, v, sizeof(v));
  return h ? h : 1;
}

static bool print_hist(const std::vector<SeqRecord> &recs, const mfx_hist_result &r, int k, const char *outName) {
  uint64_t cum = 0;
  for (size_t c = 0; c < recs.size(); ++c) {   // outputHistogram's per-sequence line, in input order
    cum += r.contig_kmissing[c];
    fprintf(stderr, "%s\t%lu\t%lu\t%lu\t%.2f\n", recs[c].name.c_str(), (unsigned long)r.contig_kmissing[c], (unsigned long)cum,
            (unsigned long)r.contig_kasm[c], mfx_histoQV((double)r.contig_kmissing[c], (double)r.contig_kasm[c], k));
  }
  return mfx_hist_report(&r, k, outName, "-") == 0;
}

static void print_completeness(const double *t64, const double *u64) {
  double total = 0, undrc = 0;
  for (int ii = 0; ii < 64; ii++) {                     // merfin-completeness.C:119-120, here in piece order
    fprintf(stderr, "thread %2u total %12.2f underc %15.5f completeness %0.8f\n", ii, t64[ii], u64[ii], 1.0 - u64[ii] / t64[ii]);
    total += t64[ii];
    undrc += u64[ii];
  }
  fprintf(stderr, "\n");
  fprintf(stderr, "TOTAL readK:   %15.2f\n", total);
  fprintf(stderr, "TOTAL undrcpy:    %15.5f\n", undrc);
  fprintf(stderr, "COMPLETENESS:             %0.5f\n", 1.0 - undrc / total);
}

// the epilogue of -count and -convert
static void print_wrote(const char *path, uint64_t n) {
  struct stat st;
  fprintf(stderr, "-- Wrote %lu k-mers", (unsigned long)n);
  if (stat(path, &st) == 0 && n) fprintf(stderr, " in %.2f GB (%.2f bytes per k-mer)", st.st_size / 1e9, (double)st.st_size / (double)n);
  fprintf(stderr, ".\n");
}

// the per-contig line of -dump and -track on stderr: name, missing k-mers, and both running sums
struct ContigCounts {
  uint64_t cumMissing = 0, cumAsm = 0;
  void line(const char *name, uint64_t kasm, uint64_t kmissing) {
    cumMissing += kmissing;
    cumAsm += kasm;
    fprintf(stderr, "%s\t%lu\t%lu\t%lu\n", name, (unsigned long)kmissing, (unsigned long)cumMissing, (unsigned long)cumAsm);
  }
  void lines(const std::vector<SeqRecord> &recs, const mfx_hist_result &r) {   // -dump -skipMissing: the counts of a -hist run
    for (size_t c = 0; c < recs.size(); ++c) line(recs[c].name.c_str(), r.contig_kasm[c], r.contig_kmissing[c]);
  }
};

// Upper bound of the bases in a sequence file WITHOUT reading it (0 = unknown): a plain file cannot hold more bases
// than bytes; a gzip file records its uncompressed size modulo 2^32 in its last four bytes (RFC 1952 ISIZE), and DNA
// text compresses 2-8x, which settles the multiple of 4 GiB.  Lets the k-mer table be sized -- and the read database
// be loaded -- while the sequence file is still being read.
static uint64_t bases_upper_bound(const char *path) {
  struct stat st;
  if (stat(path, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size <= 0) return 0;
  const uint64_t size = (uint64_t)st.st_size;
  const std::string p(path);
  auto ends = [&](const char *suf) { const size_t n = strlen(suf); return p.size() >= n && p.compare(p.size() - n, n, suf) == 0; };
  if (ends(".bz2") || ends(".xz") || ends(".zst")) return 0;
  if (!ends(".gz")) return size;
  if (size < 18) return 0;
  FILE *f = fopen(path, "rb");
  if (!f) return 0;
  unsigned char t[4];
  const bool ok = fseek(f, -4, SEEK_END) == 0 && fread(t, 1, 4, f) == 4;
  fclose(f);
  if (!ok) return 0;
  const uint64_t isize = (uint64_t)t[0] | ((uint64_t)t[1] << 8) | ((uint64_t)t[2] << 16) | ((uint64_t)t[3] << 24);
  // the largest isize + n * 2^32 that is at most 8x the compressed size (a file of several gzip members only records
  // the last member's size: then the estimate may be LOW, so it must also be at least 2x the compressed size to be used)
  uint64_t best = 0;
  for (uint64_t n = 0; n < 4096; ++n) {
    const uint64_t cand = isize + (n << 32);
    if (cand > 8 * size + (1ull << 20)) break;
    best = cand;
  }
  if (best < 2 * size) return 0;
  return best;
}

// the options of the variant modes (OP_* values are the MFX_VAR_* values); debug_path: the -debug log, or only whether it is set
static mfx_variant_opts variant_opts(const Globals &G, const char *debug_path) {
  mfx_variant_opts o;
  o.mode = G.reportType;
  o.comb = G.comb;
  o.nosplit = G.nosplit ? 1 : 0;
  o.debug_path = debug_path;
  return o;
}

// -hist and -dump with -sharded: PARTS of the assembly, one per slot (round 4).  They only ever ask the lookup tables for the
// k-mers of -sequence (merfin-histogram.C:54-64, merfin-dump.C:44-61), so a slot needs the k-mers of the contigs IT evaluates
// and nothing else: the contigs are dealt to the slots (balanced by bases), slot d claims its contigs' k-mers into a
// sequence-only index, counts them over the whole assembly (or takes them from -seqmers), the databases -- decoded once, sent
// to every slot -- update them, and every slot evaluates its contigs on its own device: no k-mer is ever exchanged, whatever
// the size of the read database (config 5: each of the 8 GPUs keeps the 1/8 of a 2 x 10^10-k-mer database that its contigs hit).
// Returns -1 when a database is not canonical (the caller falls back to the hash-sharded full tables).
static int run_parts(const Globals &G, int k, const std::vector<SeqRecord> &recs, const std::vector<const char *> &bases,
                     const std::vector<uint64_t> &lens) {
  const uint32_t N = (uint32_t)G.devices.size();
  const uint32_t NC = (uint32_t)recs.size();
  // the contigs of every slot: largest first to the least loaded slot; ascending numbers inside a slot
  std::vector<std::vector<uint32_t>> ids(N);
  {
    std::vector<uint32_t> order(NC);
    for (uint32_t c = 0; c < NC; ++c) order[c] = c;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return lens[a] > lens[b]; });
    std::vector<uint64_t> load(N, 0);
    for (uint32_t c : order) {
      const uint32_t d = (uint32_t)(std::min_element(load.begin(), load.end()) - load.begin());
      ids[d].push_back(c);
      load[d] += lens[c] + 1;
    }
    for (auto &v : ids) std::sort(v.begin(), v.end());
  }
  std::vector<mfx_index *> ixs(N, nullptr);
  std::vector<mfx_seq *> own(N, nullptr), whole(N, nullptr);
  std::vector<mfx_eval *> evs(N, nullptr);
  mfx_kparams kp{G.peak, (uint32_t)G.copyKmerK.size(), G.copyKmerK.data(), G.copyKmerP.data()};
  int rc = 0;
  auto fail = [&](const char *what) { fprintf(stderr, "ERROR: %s: %s\n", what, mfx_last_error()); rc = 1; };
  auto release = [&]() {
    for (uint32_t d = 0; d < N; ++d) {
      if (evs[d]) mfx_eval_free(evs[d]);
      if (ixs[d]) mfx_index_free(ixs[d]);
      if (own[d]) mfx_seq_free(own[d]);
      bool shared = false;
      for (uint32_t e = 0; e < d; ++e) if (whole[e] == whole[d]) shared = true;
      if (whole[d] && !shared) mfx_seq_free(whole[d]);
      evs[d] = nullptr; ixs[d] = nullptr; own[d] = nullptr; whole[d] = nullptr;
    }
  };
  for (uint32_t d = 0; d < N && !rc; ++d) {
    std::vector<const char *> b2;
    std::vector<uint64_t> l2;
    uint64_t nb = 0;
    for (uint32_t c : ids[d]) { b2.push_back(bases[c]); l2.push_back(lens[c]); nb += lens[c]; }
    fprintf(stderr, "-- Part %u of %u on device %d: %zu sequences, %lu bases.\n", d, N, G.devices[d], ids[d].size(), (unsigned long)nb);
    own[d] = mfx_seq_upload(G.devices[d], b2.data(), l2.data(), (uint32_t)b2.size());
    if (!own[d]) { fail("uploading sequences"); break; }
    ixs[d] = mfx_index_create_for_seq(k, nb + 1024, G.maxMemory, G.devices[d]);
    if (!ixs[d]) { fprintf(stderr, "\n%s\n\n", mfx_last_error()); rc = 1; break; }
    if (mfx_index_claim_seq(ixs[d], own[d], nullptr)) { fail("claiming sequence k-mers"); break; }
    if (!G.seqDBname) {
      // replaces `meryl count k=.. <seq> output <seq>.meryl` (merfin-globals.C:182-186): every contig of the assembly counts
      for (uint32_t e = 0; e < d; ++e) if (G.devices[e] == G.devices[d]) { whole[d] = whole[e]; break; }
      if (!whole[d]) whole[d] = mfx_seq_upload(G.devices[d], bases.data(), lens.data(), NC);
      if (!whole[d]) { fail("uploading sequences"); break; }
      if (mfx_index_count_claimed(ixs[d], whole[d], nullptr)) { fail("counting sequence k-mers"); break; }
    }
  }
  for (uint32_t d = 0; d < N; ++d) {                              // the whole assembly was only needed for the counts
    bool shared = false;
    for (uint32_t e = 0; e < d; ++e) if (whole[e] == whole[d]) shared = true;
    if (whole[d] && !shared) mfx_seq_free(whole[d]);
  }
  std::fill(whole.begin(), whole.end(), nullptr);
  int lrc = 0;
  if (!rc && G.seqDBname) {
    fprintf(stderr, "-- Loading kmers from '%s' into the %u parts.\n", G.seqDBname, N);
    lrc = mfx_index_load_db_multi(ixs.data(), N, G.seqDBname, 1, 0, ~0ull);
    if (lrc && lrc != MFX_E_NONCANON) fail("loading -seqmers");
  }
  if (!rc && !lrc) {
    fprintf(stderr, "-- Loading kmers from '%s' into the %u parts.\n", G.readDBname, N);
    lrc = mfx_index_load_db_multi(ixs.data(), N, G.readDBname, 0, G.minV, G.maxV);
    if (lrc && lrc != MFX_E_NONCANON) fail("loading -readmers");
  }
  if (!rc && lrc == MFX_E_NONCANON) {
    fprintf(stderr, "-- A k-mer database is not canonical; building the sharded full tables instead.\n");
    release();
    return -1;
  }
  for (uint32_t d = 0; d < N && !rc; ++d) {
    evs[d] = mfx_eval_create(ixs[d], &kp, 0);
    if (!evs[d]) { fail("creating evaluator"); break; }
  }
  std::vector<const uint32_t *> idp(N);
  for (uint32_t d = 0; d < N; ++d) idp[d] = ids[d].data();
  if (!rc && (G.reportType == OP_HIST || G.skipMissing)) {
    mfx_hist_result r;
    if (G.reportType == OP_HIST) fprintf(stderr, "-- Generate histogram of the k* metric to '%s' on %u devices (one part of the sequences each).\n", G.outName, N);
    else fprintf(stderr, "-- Dump per-base k* metric to '%s' on %u devices (one part of the sequences each).\n", G.outName, N);
    if (mfx_hist_run_parts(evs.data(), own.data(), idp.data(), N, NC, &r)) fail("-hist over the parts");
    else if (G.reportType == OP_HIST) {
      if (!print_hist(recs, r, k, G.outName)) fail("writing histogram");
      mfx_hist_result_free(&r);
    } else {                               // -dump -skipMissing (merfin-dump.C:34,81-87): no dump file, only the per-contig counts
      ContigCounts().lines(recs, r);
      mfx_hist_result_free(&r);
    }
  } else if (!rc) {
    fprintf(stderr, "-- Dump per-base k* metric to '%s' on %u devices (one part of the sequences each).\n", G.outName, N);
    // every contig by the slot that holds it, in input order (merfin.C:384: -dump writes in order)
    std::vector<std::pair<uint32_t, uint32_t>> where(NC);           // contig -> (slot, number inside the slot)
    for (uint32_t d = 0; d < N; ++d) for (uint32_t i = 0; i < ids[d].size(); ++i) where[ids[d][i]] = {d, i};
    ContigCounts counts;
    for (uint32_t c = 0; c < NC && !rc; ++c) {
      uint64_t ka = 0, km = 0;
      const uint32_t d = where[c].first;
      if (mfx_dump_contig(evs[d], own[d], where[c].second, recs[c].name.c_str(), G.outName, c > 0, &ka, &km)) { fail("-dump over the parts"); break; }
      counts.line(recs[c].name.c_str(), ka, km);
    }
    if (recs.empty()) { FILE *f = fopen(G.outName, "w"); if (f) fclose(f); }
  }
  release();
  if (!rc) fprintf(stderr, "Bye!\n");
  return rc;
}

// Every report over an index SHARDED across the devices of -devices (read databases beyond one GPU, BASELINE
// config 5): slot d keeps the k-mers it owns (mfx_index_set_shard), loads skip foreign k-mers, -hist routes every k-mer
// to its owner (mfx_hist_run_sharded), -completeness adds the per-piece sums of the shards in piece order
// (merfin-completeness.C:117-123; the sums are integer-valued, so the split is exact), -dump and the variant modes
// look every k-mer up in all shards and add the answers (mfx_dump_contig_sharded, mfx_variants_run_sharded).  The
// databases are decoded once: every batch is sent to all shards (mfx_index_load_db_multi).
static int run_sharded(const Globals &G, int k, const mfx_db_info &rdb, const mfx_db_info &adb, const std::vector<SeqRecord> &recs,
                       const std::vector<const char *> &bases, const std::vector<uint64_t> &lens, const std::vector<const char *> &names,
                       uint64_t totalBases) {
  const uint32_t N = (uint32_t)G.devices.size();
  std::vector<mfx_index *> ixs(N, nullptr);
  std::vector<mfx_seq *> sqs(N, nullptr);
  std::vector<mfx_eval *> evs(N, nullptr);
  std::vector<mfx_router *> rts(N, nullptr);
  mfx_kparams kp{G.peak, (uint32_t)G.copyKmerK.size(), G.copyKmerK.data(), G.copyKmerP.data()};
  const uint64_t whole = rdb.n_kmers + (G.seqDBname ? adb.n_kmers : totalBases) + 1024;
  const uint64_t capacity = (uint64_t)((double)whole / N * 1.15) + 1024;      // owners are hash-balanced
  int rc = 0;
  auto fail = [&](const char *what) { fprintf(stderr, "ERROR: %s: %s\n", what, mfx_last_error()); rc = 1; };
  for (uint32_t d = 0; d < N && !rc; ++d) {
    uint32_t same = d;
    for (uint32_t e = 0; e < d; ++e) if (G.devices[e] == G.devices[d]) { same = e; break; }
    if (!recs.empty() || G.seqName) {
      sqs[d] = same < d ? sqs[same] : mfx_seq_upload(G.devices[d], bases.data(), lens.data(), (uint32_t)recs.size());
      if (!sqs[d]) { fail("uploading sequences"); break; }
    }
    fprintf(stderr, "-- Shard %u of %u on device %d.\n", d, N, G.devices[d]);
    ixs[d] = mfx_index_create(k, capacity, G.maxMemory, G.devices[d]);
    if (!ixs[d]) { fprintf(stderr, "\n%s\n\n", mfx_last_error()); rc = 1; break; }
    if (mfx_index_set_shard(ixs[d], d, N)) { fail("creating shard"); break; }
  }
  // one pass over each database feeds every shard (each keeps the k-mers it owns)
  if (!rc) {
    fprintf(stderr, "-- Loading kmers from '%s' into the %u shards.\n", G.readDBname, N);
    if (mfx_index_load_db_multi(ixs.data(), N, G.readDBname, 0, G.minV, G.maxV)) fail("loading -readmers");
  }
  if (!rc && G.seqDBname) {
    fprintf(stderr, "-- Loading kmers from '%s' into the %u shards.\n", G.seqDBname, N);
    if (mfx_index_load_db_multi(ixs.data(), N, G.seqDBname, 1, 0, ~0ull)) fail("loading -seqmers");
  }
  for (uint32_t d = 0; d < N && !rc; ++d) {
    if (!G.seqDBname && mfx_index_count_asm(ixs[d], sqs[d], nullptr)) { fail("counting sequence k-mers"); break; }
    evs[d] = mfx_eval_create(ixs[d], &kp, 0);
    if (!evs[d]) { fail("creating evaluator"); break; }
    if (G.reportType == OP_HIST || (G.reportType == OP_DUMP && G.skipMissing)) {
      const uint64_t nt = mfx_seq_num_tiles(sqs[d]);
      rts[d] = mfx_router_create(ixs[d], N, (uint32_t)std::min<uint64_t>(16384, std::max<uint64_t>(1, nt)));
      if (!rts[d]) { fail("creating router"); break; }
    }
  }
  if (!rc && G.reportType == OP_HIST) {
    fprintf(stderr, "-- Generate histogram of the k* metric to '%s' on %u devices (sharded index).\n", G.outName, N);
    mfx_hist_result r;
    if (mfx_hist_run_sharded(evs.data(), rts.data(), sqs.data(), N, &r)) fail("-hist over the sharded index");
    else {
      if (!print_hist(recs, r, k, G.outName)) fail("writing histogram");
      mfx_hist_result_free(&r);
    }
  } else if (!rc && G.reportType == OP_DUMP) {
    fprintf(stderr, "-- Dump per-base k* metric to '%s' on %u devices (sharded index).\n", G.outName, N);
    ContigCounts counts;
    if (G.skipMissing) {                 // merfin-dump.C:34,81-87: no dump file, only the per-contig counts
      mfx_hist_result r;
      if (mfx_hist_run_sharded(evs.data(), rts.data(), sqs.data(), N, &r)) fail("-dump -skipMissing over the sharded index");
      else {
        counts.lines(recs, r);
        mfx_hist_result_free(&r);
      }
    } else {
      for (size_t c = 0; c < recs.size() && !rc; ++c) {
        uint64_t ka = 0, km = 0;
        if (mfx_dump_contig_sharded(evs.data(), sqs.data(), N, (uint32_t)c, recs[c].name.c_str(), G.outName, c > 0, &ka, &km)) { fail("-dump over the sharded index"); break; }
        counts.line(recs[c].name.c_str(), ka, km);
      }
      if (recs.empty()) { FILE *f = fopen(G.outName, "w"); if (f) fclose(f); }
    }
  } else if (!rc && G.reportType >= OP_FILTER) {
    fprintf(stderr, "-- Opening vcf file '%s'.\n", G.vcfName);
    fprintf(stderr, "-- Generate variant mers and score them on %u devices (sharded index).\n", N);
    const std::string outName = std::string(G.outName) + (G.reportType == OP_POLISH ? ".polish.vcf" : ".filter.vcf");   // merfin-variants.C:324-327
    const std::string dbgName = std::string(G.outName) + ".00.debug.gz";
    const mfx_variant_opts vo = variant_opts(G, G.debug ? dbgName.c_str() : nullptr);
    uint64_t ncl = 0;
    if (mfx_variants_run_sharded(evs.data(), N, G.vcfName, names.data(), bases.data(), lens.data(), (uint32_t)recs.size(), &vo, outName.c_str(), nullptr, &ncl))
      fail("variant scoring over the sharded index");
  } else if (!rc) {
    fprintf(stderr, "-- Compute completeness on %u devices (sharded index).\n", N);
    double t64[64] = {0}, u64[64] = {0};
    for (uint32_t d = 0; d < N && !rc; ++d) {
      double t[64], u[64];
      if (mfx_completeness_pieces(evs[d], t, u)) { fail("-completeness"); break; }
      for (int i = 0; i < 64; ++i) { t64[i] += t[i]; u64[i] += u[i]; }
    }
    if (!rc) print_completeness(t64, u64);
  }
  for (uint32_t d = 0; d < N; ++d) {
    if (rts[d]) mfx_router_free(rts[d]);
    if (evs[d]) mfx_eval_free(evs[d]);
    if (ixs[d]) mfx_index_free(ixs[d]);
    bool shared = false;
    for (uint32_t e = 0; e < d; ++e) if (G.devices[e] == G.devices[d]) shared = true;
    if (sqs[d] && !shared) mfx_seq_free(sqs[d]);
  }
  if (!rc) fprintf(stderr, "Bye!\n");
  return rc;
}

// One evaluation context per entry of -devices: slot 0 is the index / sequence / evaluator the run built, the others
// are replicas made by peer copy (a device named twice shares table and sequence; every slot has its own evaluator).
struct Slots {
  std::vector<mfx_index *> ixs;
  std::vector<mfx_seq *> sqs;
  std::vector<mfx_eval *> evs;
  std::vector<int> devs;
  bool make(const Globals &G, mfx_index *ix, mfx_seq *seq, mfx_eval *ev, const mfx_kparams *kp) {
    const size_t N = G.devices.size();
    devs = G.devices;
    ixs.assign(N, nullptr); sqs.assign(N, nullptr); evs.assign(N, nullptr);
    ixs[0] = ix; sqs[0] = seq; evs[0] = ev;
    // the devices that need a copy (a device named twice shares table and sequence): all at once, by a doubling tree
    std::vector<int> fresh;
    std::vector<size_t> first(N, 0);
    for (size_t d = 0; d < N; ++d) {
      first[d] = d;
      for (size_t e = 0; e < d; ++e) if (devs[e] == devs[d]) { first[d] = e; break; }
      if (first[d] == d && d > 0) fresh.push_back(devs[d]);
    }
    std::vector<mfx_index *> rix(fresh.size(), nullptr);
    std::vector<mfx_seq *> rsq(fresh.size(), nullptr);
    if (!fresh.empty()) {
      if (mfx_index_replicate_many(ix, fresh.data(), (uint32_t)fresh.size(), rix.data())) return false;
      if (seq && mfx_seq_replicate_many(seq, fresh.data(), (uint32_t)fresh.size(), rsq.data())) {
        for (auto *x : rix) mfx_index_free(x);
        return false;
      }
    }
    for (size_t d = 1, f = 0; d < N; ++d) {
      if (first[d] == d) { ixs[d] = rix[f]; sqs[d] = rsq[f]; ++f; }
      else { ixs[d] = ixs[first[d]]; sqs[d] = sqs[first[d]]; }
    }
    for (size_t d = 1; d < N; ++d) {
      evs[d] = mfx_eval_create(ixs[d], kp, 0);
      if (!evs[d]) { release(); return false; }
    }
    return true;
  }
  void release() {                       // slot 0 belongs to the caller
    for (size_t d = 1; d < ixs.size(); ++d) {
      if (evs[d]) mfx_eval_free(evs[d]);
      bool shared = false;
      for (size_t e = 0; e < d; ++e) if (devs[e] == devs[d]) shared = true;
      if (!shared) { if (sqs[d]) mfx_seq_free(sqs[d]); if (ixs[d]) mfx_index_free(ixs[d]); }
    }
    evs.clear(); ixs.clear(); sqs.clear();
  }
};

// contiguous split of the contigs (input order) into `parts` runs of about equal weight; every slot works on its run
// and the outputs are concatenated in slot order -- the reference's SLURM-array recipe (scripts/parallel1/merfin.sh:68-85)
static std::vector<std::pair<size_t, size_t>> contig_partition(const std::vector<double> &w, size_t parts) {
  const size_t n = w.size();
  std::vector<double> cum(n + 1, 0.0);
  for (size_t i = 0; i < n; ++i) cum[i + 1] = cum[i] + w[i];
  std::vector<size_t> cuts(1, 0);
  for (size_t r = 1; r < parts; ++r) {
    size_t c = cum[n] > 0 ? (size_t)(std::lower_bound(cum.begin(), cum.end(), cum[n] * (double)r / (double)parts) - cum.begin()) : n * r / parts;
    cuts.push_back(std::min(n, std::max(cuts.back(), c)));
  }
  cuts.push_back(n);
  std::vector<std::pair<size_t, size_t>> out;
  for (size_t r = 0; r < parts; ++r) out.emplace_back(cuts[r], cuts[r + 1]);
  return out;
}

// parts -> out (slot order); skip_header: the '#' lines of every part but the first are dropped (VCF)
static bool concat_parts(const std::string &out, const std::vector<std::string> &parts, bool skip_header) {
  FILE *o = fopen(out.c_str(), "wb");
  if (!o) return false;
  std::vector<char> buf(1 << 22);
  bool ok = true;
  for (size_t i = 0; i < parts.size() && ok; ++i) {
    FILE *f = fopen(parts[i].c_str(), "rb");
    if (!f) continue;                                         // a slot without contigs wrote nothing
    bool at_line_start = true, in_header = false;
    size_t n;
    while ((n = fread(buf.data(), 1, buf.size(), f)) > 0 && ok) {
      if (!(skip_header && i > 0)) { ok = fwrite(buf.data(), 1, n, o) == n; continue; }
      size_t b = 0;                                           // copy everything except lines starting with '#'
      for (size_t j = 0; j < n; ++j) {
        if (at_line_start) {
          if (!in_header && j > b) ok = ok && fwrite(buf.data() + b, 1, j - b, o) == j - b;
          in_header = buf[j] == '#';
          b = j;
          at_line_start = false;
        }
        if (buf[j] == '\n') {
          at_line_start = true;
          if (in_header) b = j + 1;
        }
      }
      if (!in_header && n > b) ok = ok && fwrite(buf.data() + b, 1, n - b, o) == n - b;
      if (in_header) b = n;
    }
    fclose(f);
    remove(parts[i].c_str());
  }
  return fclose(o) == 0 && ok;
}

// The records of the -reads files to `sink`, batch after batch: one reader thread per file (16 at most at a time) parses records into
// batches of about 16 M bases; this thread hands them to sink(bases, lens, n), which returns 0 to go on.  Anything else stops the readers
// and ends the call with that value (the sink keeps its own error text).  FEED_FILE_FAILED, no value of a sink or of the library: a file failed,
// and `file_why`, which only the readers write, under the lock, says how.  t_wait: seconds this thread waited for parsed records.
constexpr int FEED_FILE_FAILED = 1 << 20;
template <class Sink>
static int feed_reads_files(const Globals &G, Sink &&sink, std::string &file_why, double *t_wait_out = nullptr) {
  constexpr uint64_t BATCH_BASES = 16ull << 20;
  std::mutex mu;
  std::condition_variable cv_full, cv_room;
  std::deque<std::vector<SeqRecord>> queue;
  const size_t nfiles = G.readsNames.size(), nthreads = std::min<size_t>(16, nfiles), max_queued = 2 * nthreads + 2;
  size_t running = nthreads;
  std::atomic<size_t> next_file{0};
  std::atomic<bool> failed{false};
  int result = 0;
  auto push = [&](std::vector<SeqRecord> &b) {
    std::unique_lock<std::mutex> lk(mu);
    cv_room.wait(lk, [&] { return queue.size() < max_queued || failed.load(); });
    queue.push_back(std::move(b));
    cv_full.notify_one();
    b.clear();
  };
  std::vector<std::thread> readers;
  for (size_t t = 0; t < nthreads; ++t)
    readers.emplace_back([&]() {
      for (size_t f; !failed.load() && (f = next_file++) < nfiles;) {
        SeqFile sf(G.readsNames[f]);
        if (!sf.ok()) {
          std::lock_guard<std::mutex> lk(mu);
          file_why = std::string("cannot open '") + G.readsNames[f] + "'";
          failed = true;
          result = FEED_FILE_FAILED;
          break;
        }
        std::vector<SeqRecord> batch;
        uint64_t held = 0;
        for (SeqRecord r; sf.next(r); r = SeqRecord()) {
          held += r.size();
          batch.push_back(std::move(r));
          if (held >= BATCH_BASES) { push(batch); held = 0; }
          if (failed.load()) break;
        }
        if (!batch.empty()) push(batch);
        if (sf.finish() != 0) {
          std::lock_guard<std::mutex> lk(mu);
          if (!failed.load()) {                                          // (a reader stopped on purpose ends its decompressor early: no finding)
            file_why = std::string("reading '") + G.readsNames[f] + "' failed (read error, or the decompressor exited with an error)";
            failed = true;
            result = FEED_FILE_FAILED;
          }
        }
      }
      std::lock_guard<std::mutex> lk(mu);
      --running;
      cv_full.notify_all();
    });
  double t_wait = 0;
  std::vector<const char *> ptrs;
  std::vector<uint64_t> lens;
  while (true) {
    std::vector<SeqRecord> b;
    {
      const auto tw = std::chrono::steady_clock::now();
      std::unique_lock<std::mutex> lk(mu);
      cv_full.wait(lk, [&] { return !queue.empty() || running == 0; });
      t_wait += std::chrono::duration<double>(std::chrono::steady_clock::now() - tw).count();
      if (queue.empty()) break;
      b = std::move(queue.front());
      queue.pop_front();
      cv_room.notify_one();
    }
    if (failed.load()) continue;                                   // (drain: the readers finish their pushes)
    ptrs.resize(b.size());
    lens.resize(b.size());
    for (size_t i = 0; i < b.size(); ++i) { ptrs[i] = b[i].data(); lens[i] = b[i].size(); }
    const int src = sink(ptrs.data(), lens.data(), (uint64_t)b.size());
    if (src) {
      std::lock_guard<std::mutex> lk(mu);
      if (!failed.load()) result = src;
      failed = true;
      cv_room.notify_all();
    }
  }
  for (auto &t : readers) t.join();
  if (t_wait_out) *t_wait_out = t_wait;
  return result;
}

// -reads: the read counts of the run from its reads, counted on the device into the k-mers the index holds (mfx_reads_*).  The reader
// threads parse (feed_reads_files); this thread hands the batches to the counter, which copies them and returns while the device counts,
// so parsing, transfer and counting overlap.  Returns false with the error printed.
// all (-count): the claiming counter -- every k-mer of the reads, no filter; *all_stats gets its statistics and the caller reports.
// range (-count -passes): the claiming counter over the k-mers of [range[0], range[1]); batch: its bases per device batch (0: the library's).
// fail_code: where to put the code of a failing counter INSTEAD of printing the error (the text stays in `fail_text`).
static bool count_reads_files(const Globals &G, mfx_index *ix, bool all = false, mfx_reads_stats *all_stats = nullptr, uint64_t batch = 0,
                              const uint64_t *range = nullptr, int *fail_code = nullptr, std::string *fail_text = nullptr) {
  const auto t0 = std::chrono::steady_clock::now();
  mfx_reads *rc = range ? mfx_reads_begin_range(ix, batch, range[0], range[1]) : all ? mfx_reads_begin_all(ix, batch) : mfx_reads_begin(ix, 0);
  if (!rc || mfx_reads_set_filter(rc, all ? 0 : G.minV, all ? ~0ull : G.maxV)) {
    fprintf(stderr, "ERROR: counting -reads: %s\n", mfx_last_error());
    if (rc) mfx_reads_end(rc, nullptr);
    return false;
  }
  double t_wait = 0, t_submit = 0;
  std::string file_why, add_why;                                 // (the readers write the first, this thread the second)
  const int frc = feed_reads_files(G, [&](const char *const *bases, const uint64_t *lens, uint64_t n) {
    const auto ts = std::chrono::steady_clock::now();
    const int arc = mfx_reads_add(rc, bases, lens, n);
    t_submit += std::chrono::duration<double>(std::chrono::steady_clock::now() - ts).count();
    if (arc) add_why = mfx_last_error();
    return arc;
  }, file_why, &t_wait);
  mfx_reads_stats st;
  const int erc = mfx_reads_end(rc, &st);
  if (frc || erc) {
    const bool file_failed = frc == FEED_FILE_FAILED;
    const int code = file_failed ? MFX_E_IO : frc ? frc : erc;   // (frc otherwise: the code of the mfx_reads_add that failed)
    const std::string text = file_failed ? file_why : frc ? add_why : std::string(mfx_last_error());
    if (fail_code && !file_failed) {
      *fail_code = code;
      if (fail_text) *fail_text = text;
      return false;
    }
    fprintf(stderr, "ERROR: counting -reads: %s\n", text.c_str());
    if (fail_code) *fail_code = MFX_OK;
    return false;
  }
  const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (all_stats) *all_stats = st;
  if (!all)
    fprintf(stderr, "-- Counted the %d-mers of %lu reads (%lu bases): %lu k-mers, %lu counted, %lu dropped.\n", G.kArg, (unsigned long)st.reads,
            (unsigned long)st.bases, (unsigned long)st.kmers, (unsigned long)st.counted, (unsigned long)st.dropped);
  if (env_flag("MFX_CLI_TIMING") > 0)
    fprintf(stderr, "-- reads: %.3f s wall = %.3f s waiting for parsed records + %.3f s batching / encoding / waiting for a stage; device %.3f s kernel + "
                    "%.3f s copy (idle %.0f %% of the wall)\n", wall, t_wait, t_submit, st.seconds_kernel, st.seconds_copy,
            wall > 0 ? 100.0 * std::max(0.0, 1.0 - (st.seconds_kernel + st.seconds_copy) / wall) : 0.0);
  return true;
}

#define DIE_MFX(what)                                                       \
  do {                                                                      \
    fprintf(stderr, "ERROR: %s: %s\n", what, mfx_last_error());             \
    return 1;                                                               \
  } while (0)

// ---- -count -passes: the k-mers of the reads counted in passes over ascending key ranges ------------------------------------------------
// A range is [bin_lo, bin_hi) of the 2^min(2k, 12) bins of the top key bits (mfx_index_key_bins).  Every pass counts its range into an index
// of its own, created at 1024 lines under -memory (mfx_reads_begin_range), and appends the table to one writer (mfx_db_writer_*): ascending
// ranges append into the file of one pass, byte for byte.  A range whose table cannot grow (MFX_E_NOMEM) is cut in two at the bins of the
// table it reached (mfx_cut_bins) and both halves are queued.  The reads are parsed once into a read store (mfx_reads_store_*) beside
// pass 1 and replayed from it afterwards; without a store (MFX_COUNT_STORE_GB=0, or one that filled up) every pass reads the files.
namespace {
struct CountPasses {
  const Globals &G;
  uint64_t batch = 0;                                            // MFX_COUNT_BATCH
  uint32_t nbins = 0;
  int shift = 0;
  std::deque<std::pair<uint32_t, uint32_t>> todo;                // the ranges to count, ascending
  mfx_db_writer *w = nullptr;
  uint64_t n_pass = 0, n_refused = 0, distinct = 0, counted = 0, growths = 0;
  double max_gb = 0;
  mfx_reads_stats first{};                                       // the statistics of the first pass that ended: reads, bases, k-mers
  bool have_first = false;
  // the pass that runs
  mfx_index *ix = nullptr;
  mfx_reads *r = nullptr;
  std::pair<uint32_t, uint32_t> cur{0, 0};
  std::chrono::steady_clock::time_point t0;

  explicit CountPasses(const Globals &g) : G(g) {}
  ~CountPasses() {
    if (r) mfx_reads_end(r, nullptr);
    if (ix) mfx_index_free(ix);
    if (w) mfx_db_writer_abort(w);
  }
  uint64_t key_of(uint32_t bin) const { return (uint64_t)bin << shift; }     // (bin == nbins: 4^k)

  // the next range of the queue gets its index and its counter; false: the error is printed
  bool begin() {
    cur = todo.front();
    todo.pop_front();
    t0 = std::chrono::steady_clock::now();
    ix = mfx_index_create(G.kArg, 1024, G.maxMemory, G.device);
    if (!ix) { fprintf(stderr, "ERROR: creating the k-mer table: %s\n", mfx_last_error()); return false; }
    r = mfx_reads_begin_range(ix, batch, key_of(cur.first), key_of(cur.second));
    if (!r) { fprintf(stderr, "ERROR: counting -reads: %s\n", mfx_last_error()); return false; }
    return true;
  }
  // the pass's table could not grow: its range is cut in two at the bins of what it holds.  false: a range of one bin -- the library's text ends the run
  bool refuse(const std::string &text) {
    if (cur.second - cur.first < 2) {
      fprintf(stderr, "ERROR: counting -reads: %s\n", text.c_str());
      fprintf(stderr, "-- The key range that does not fit is one bin of %u (bin %u): no pass can be smaller.  Increase -memory.\n", nbins, cur.first);
      return false;
    }
    std::vector<uint64_t> bins(4096);
    std::vector<mfx_bin_range> halves;
    if (mfx_index_key_bins(ix, 0, bins.data(), nullptr) == MFX_OK) mfx_cut_bins(bins.data(), cur.first, cur.second, 2, halves);
    const uint32_t cut = halves.size() == 2 ? halves[0].bin_hi : cur.first + (cur.second - cur.first) / 2;   // (entries in one bin only so far: the middle)
    fprintf(stderr, "-- Bins [%u, %u) of %u: refused, the table could not grow beyond %.6f GB; cut in two at bin %u.\n", cur.first, cur.second, nbins,
            table_gb(), cut);
    mfx_index_free(ix);
    ix = nullptr;
    todo.push_front({cut, cur.second});
    todo.push_front({cur.first, cut});
    ++n_refused;
    return true;
  }
  double table_gb() const {
    mfx_index_info info;
    return ix && mfx_index_get_info(ix, &info) == MFX_OK ? (double)info.bytes / 1e9 : 0.0;
  }
  // the counter of the running pass ends.  1: done, its table appended; 0: refused and cut in two; -1: failed, the error is printed
  int finish(const char *source) {
    mfx_reads_stats st;
    const int erc = mfx_reads_end(r, &st);
    r = nullptr;
    if (erc == MFX_E_NOMEM) return refuse(mfx_last_error()) ? 0 : -1;
    if (erc) { fprintf(stderr, "ERROR: counting -reads: %s\n", mfx_last_error()); return -1; }
    return append(st, source) ? 1 : -1;
  }
  bool append(const mfx_reads_stats &st, const char *source) {
    mfx_index_info info;
    uint64_t g = 0, added = 0;
    if (mfx_index_get_info(ix, &info) || mfx_index_growths(ix, &g, nullptr, nullptr, nullptr)) { fprintf(stderr, "ERROR: -count: %s\n", mfx_last_error()); return false; }
    if (mfx_db_writer_append_index(w, ix, 0, &added)) { fprintf(stderr, "ERROR: -count: collecting the k-mers of a pass: %s\n", mfx_last_error()); return false; }
    mfx_index_free(ix);
    ix = nullptr;
    if (!have_first) { first = st; have_first = true; }
    ++n_pass;
    distinct += added;
    counted += st.counted;
    growths += g;
    max_gb = std::max(max_gb, (double)info.bytes / 1e9);
    fprintf(stderr, "-- Pass %lu: bins [%u, %u) of %u: %lu k-mers counted, %lu distinct, table %.3f GB, %.2f s, %s.\n", (unsigned long)n_pass, cur.first,
            cur.second, nbins, (unsigned long)st.counted, (unsigned long)added, (double)info.bytes / 1e9,
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), source);
    return true;
  }
};

// half of MemAvailable, in bytes (0: unknown)
static uint64_t half_of_available_memory() {
  FILE *f = fopen("/proc/meminfo", "r");
  if (!f) return 0;
  char line[256];
  unsigned long long kb = 0;
  while (fgets(line, sizeof(line), f))
    if (sscanf(line, "MemAvailable: %llu kB", &kb) == 1) break;
  fclose(f);
  return (uint64_t)kb * 1024 / 2;
}
}  // namespace

// the writer of -count: the streamed one (the blocks are coded on the device and go to disk as they are made) unless MFX_COUNT_WRITER=host
// asks for the one that collects the k-mers on the host (docs/KNOBS.md); both write the same bytes.  -1: the knob holds something else
static int count_writer_streamed() {
  if (const char *e = getenv("MFX_COUNT_WRITER")) {
    if (!strcmp(e, "host")) return 0;
    if (!strcmp(e, "stream")) return 1;
    fprintf(stderr, "ERROR: -count: MFX_COUNT_WRITER is 'stream' or 'host', not '%s'.\n", e);
    return -1;
  }
  const char *de = getenv("MFX_FLAT_DELTA");                      // (another form than delta-coded blocks: only the host writer makes it)
  return !(de && atoi(de) == 0);
}

static int count_in_passes(const Globals &G) {
  const int streamed = count_writer_streamed();
  if (streamed < 0) return 1;
  CountPasses C(G);
  if (const char *e = getenv("MFX_COUNT_BATCH")) C.batch = strtoull(e, nullptr, 10);
  const int bits = std::min(2 * G.kArg, 12);
  C.nbins = 1u << bits;
  C.shift = 2 * G.kArg - bits;
  uint64_t store_bytes = half_of_available_memory();
  if (const char *e = getenv("MFX_COUNT_STORE_GB")) store_bytes = (uint64_t)(std::max(0.0, strtod(e, nullptr)) * 1e9);
  const uint32_t P = G.passesAuto ? 1 : G.passes;
  C.w = streamed ? mfx_db_writer_open_streamed(G.outName, G.kArg) : mfx_db_writer_open(G.outName, G.kArg);
  if (!C.w) DIE_MFX("-count");
  struct StoreGuard { mfx_reads_store *s; ~StoreGuard() { if (s) mfx_reads_store_free(s); } } SG{nullptr};
  if (store_bytes) {
    SG.s = mfx_reads_store_create(G.kArg, C.batch, store_bytes);
    if (!SG.s) DIE_MFX("-count: the read store");
  }
  std::vector<uint64_t> bins(4096);
  std::vector<mfx_bin_range> cuts;
  // the P ranges from the k-mers of the pilot: `replay` sends them through a claiming counter of a throw-away index
  auto ranges_from_pilot = [&](auto &&count_pilot) {
    C.todo.clear();
    mfx_index *pix = P > 1 ? mfx_index_create(G.kArg, 1024, G.maxMemory, G.device) : nullptr;
    if (pix && count_pilot(pix) && mfx_index_key_bins(pix, 0, bins.data(), nullptr) == MFX_OK) {
      mfx_cut_bins(bins.data(), 0, C.nbins, P, cuts);
      for (const auto &c : cuts) C.todo.push_back({c.bin_lo, c.bin_hi});
    }
    if (pix) mfx_index_free(pix);
    if (C.todo.empty()) C.todo.push_back({0u, C.nbins});           // one pass, or a pilot that showed nothing: the refusals cut from here
  };
  bool from_store = SG.s != nullptr;
  if (from_store) {
    // ---- the files are parsed once: the store fills, pass 1 counts every batch as it is complete
    uint64_t sent = 0;                                             // batches of the store pass 1 has taken
    bool started = false, pass1 = false;
    int fatal = 0;
    auto pilot = [&](mfx_index *pix) {
      mfx_reads *pr = mfx_reads_begin_all(pix, C.batch);
      if (!pr) return false;
      const int rrc = mfx_reads_replay(pr, SG.s, 0, 1);
      return mfx_reads_end(pr, nullptr) == MFX_OK && rrc == MFX_OK;
    };
    // batches [sent, upto) through pass 1; a refusal ends pass 1 (its halves are queued) and the store goes on filling
    auto advance = [&](uint64_t upto) {
      if (!started && upto > 0) {
        started = true;
        ranges_from_pilot(pilot);
        pass1 = C.begin();
        if (!pass1) { fatal = 1; return; }
      }
      if (!pass1 || upto <= sent) return;
      const int rrc = mfx_reads_replay(C.r, SG.s, sent, upto - sent);
      sent = upto;
      if (rrc == MFX_OK) return;
      pass1 = false;
      if (C.finish("from memory") < 0) fatal = 1;                  // (MFX_E_NOMEM: refused and cut; anything else is printed)
    };
    std::string file_why, store_why;
    const int frc = feed_reads_files(G, [&](const char *const *bases, const uint64_t *lens, uint64_t n) {
      const int arc = mfx_reads_store_add(SG.s, bases, lens, n);
      if (arc) { if (arc < 0) store_why = mfx_last_error(); return arc; }
      uint64_t held = 0;
      mfx_reads_store_info(SG.s, &held, nullptr, nullptr, nullptr, nullptr);
      if (held > 1) advance(held - 1);                             // (the last batch is still being filled)
      return fatal ? 2 : 0;
    }, file_why);
    if (frc == 2 || fatal) return 1;
    if (frc == FEED_FILE_FAILED || frc < 0) { fprintf(stderr, "ERROR: counting -reads: %s\n", (frc < 0 ? store_why : file_why).c_str()); return 1; }
    if (frc == 1) {                                                // the store is full: every pass reads the files
      fprintf(stderr, "-- The read store is full at %.3f GB (MFX_COUNT_STORE_GB): every pass reads the files.\n", (double)store_bytes / 1e9);
      if (C.r) { mfx_reads_end(C.r, nullptr); C.r = nullptr; }
      if (C.ix) { mfx_index_free(C.ix); C.ix = nullptr; }
      mfx_reads_store_free(SG.s);
      SG.s = nullptr;
      from_store = false;
      C.n_refused = 0;
    } else {
      uint64_t held = 0;
      mfx_reads_store_info(SG.s, &held, nullptr, nullptr, nullptr, nullptr);
      if (!started && held == 0) ranges_from_pilot([](mfx_index *) { return false; });      // no k-mer in the files: one pass over nothing
      advance(held);
      if (fatal) return 1;
      if (pass1 && C.finish("from memory") < 0) return 1;
      while (!C.todo.empty()) {
        if (!C.begin()) return 1;
        const int rrc = mfx_reads_replay(C.r, SG.s, 0, held);
        if (rrc != MFX_OK && rrc != MFX_E_NOMEM) { fprintf(stderr, "ERROR: counting -reads: %s\n", mfx_last_error()); return 1; }
        if (C.finish("from memory") < 0) return 1;
      }
    }
  }
  if (!from_store) {
    // ---- no store: the pilot is the first batch of the first file's records, every pass reads the files
    if (C.n_pass == 0) {
      auto pilot = [&](mfx_index *pix) {
        mfx_reads *pr = mfx_reads_begin_all(pix, C.batch);
        if (!pr) return false;
        mfx_reads_store *one = mfx_reads_store_create(G.kArg, C.batch, 0);
        std::string why;
        bool ok = one != nullptr;
        if (ok) {
          feed_reads_files(G, [&](const char *const *bases, const uint64_t *lens, uint64_t n) {
            uint64_t held = 0;
            if (mfx_reads_store_add(one, bases, lens, n)) return 3;
            mfx_reads_store_info(one, &held, nullptr, nullptr, nullptr, nullptr);
            return held > 1 ? 3 : 0;                               // the first batch is complete: enough
          }, why);
          uint64_t held = 0;
          mfx_reads_store_info(one, &held, nullptr, nullptr, nullptr, nullptr);
          ok = held > 0 && mfx_reads_replay(pr, one, 0, 1) == MFX_OK;
        }
        if (one) mfx_reads_store_free(one);
        return mfx_reads_end(pr, nullptr) == MFX_OK && ok;
      };
      ranges_from_pilot(pilot);
    }
    while (!C.todo.empty()) {
      C.cur = C.todo.front();
      C.todo.pop_front();
      C.t0 = std::chrono::steady_clock::now();
      C.ix = mfx_index_create(G.kArg, 1024, G.maxMemory, G.device);
      if (!C.ix) DIE_MFX("creating the k-mer table");
      const uint64_t range[2] = {C.key_of(C.cur.first), C.key_of(C.cur.second)};
      mfx_reads_stats st;
      int code = MFX_OK;
      std::string text;
      if (!count_reads_files(G, C.ix, true, &st, C.batch, range, &code, &text)) {
        if (code != MFX_E_NOMEM) {
          if (code != MFX_OK) fprintf(stderr, "ERROR: counting -reads: %s\n", text.c_str());
          return 1;
        }
        if (!C.refuse(text)) return 1;
        continue;
      }
      if (!C.append(st, "from the files")) return 1;
    }
  }
  if (C.have_first && C.counted != C.first.kmers) {
    fprintf(stderr, "ERROR: -count: the passes counted %lu of the reads' %lu k-mers\n", (unsigned long)C.counted, (unsigned long)C.first.kmers);
    return 1;
  }
  fprintf(stderr, "-- Counted the %d-mers of %lu reads (%lu bases): %lu k-mers, %lu distinct; the table grew %lu time%s to %.3f GB in %lu pass%s (%lu refused and split).\n",
          G.kArg, (unsigned long)C.first.reads, (unsigned long)C.first.bases, (unsigned long)C.first.kmers, (unsigned long)C.distinct, (unsigned long)C.growths,
          C.growths == 1 ? "" : "s", C.max_gb, (unsigned long)C.n_pass, C.n_pass == 1 ? "" : "es", (unsigned long)C.n_refused);
  const auto tw0 = std::chrono::steady_clock::now();
  uint64_t n = 0;
  mfx_db_writer *w = C.w;
  C.w = nullptr;
  if (mfx_db_writer_close(w, &n)) DIE_MFX("-count: writing the database");
  print_wrote(G.outName, n);
  if (env_flag("MFX_CLI_TIMING") > 0)
    fprintf(stderr, "-- count: %.3f s writing\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - tw0).count());
  fprintf(stderr, "Bye!\n");
  return 0;
}

// what a run owns, released on every way out
template <class T, void (*Free)(T *)>
struct Owned {
  T *p = nullptr;
  Owned() = default;
  Owned(const Owned &) = delete;
  ~Owned() { reset(); }
  void reset(T *q = nullptr) { if (p) Free(p); p = q; }
  Owned &operator=(T *q) { reset(q); return *this; }
  T *release() { T *q = p; p = nullptr; return q; }
  operator T *() const { return p; }
};
// a call set that a thread of its own loads: waited for, and freed if nobody took it
struct VcfFuture {
  std::future<mfx_vcf *> f;
  ~VcfFuture() { if (f.valid()) mfx_vcf_free(f.get()); }
};

// ---- the operations that are not reports ----------------------------------------------------------------------------------------------
// merfin -count -reads <files> -k K -output <file>: the table is created small and grows with what the reads hold (mfx_reads_begin_all)
static int run_count(Globals &G) {
  if (!G.devices.empty()) G.device = G.devices[0];
  if (!devices_available({G.device})) return 1;
  if (G.passesGiven) {
    fprintf(stderr, "-- Counting the %d-mers of %lu -reads file%s in passes over key ranges.\n", G.kArg, (unsigned long)G.readsNames.size(),
            G.readsNames.size() == 1 ? "" : "s");
    return count_in_passes(G);
  }
  const int streamed = count_writer_streamed();
  if (streamed < 0) return 1;
  const auto tc0 = std::chrono::steady_clock::now();
  uint64_t count_batch = 0;                                      // MFX_COUNT_BATCH (docs/KNOBS.md): bases per device batch; unset: the library's
  if (const char *e = getenv("MFX_COUNT_BATCH")) count_batch = strtoull(e, nullptr, 10);
  Owned<mfx_index, mfx_index_free> ix;
  ix = mfx_index_create(G.kArg, 1024, G.maxMemory, G.device);
  if (!ix) DIE_MFX("creating the k-mer table");
  fprintf(stderr, "-- Counting the %d-mers of %lu -reads file%s.\n", G.kArg, (unsigned long)G.readsNames.size(), G.readsNames.size() == 1 ? "" : "s");
  mfx_reads_stats st;
  int count_code = MFX_OK;
  std::string count_text;
  if (!count_reads_files(G, ix, true, &st, count_batch, nullptr, &count_code, &count_text)) {
    if (count_code != MFX_OK) fprintf(stderr, "ERROR: counting -reads: %s\n", count_text.c_str());
    if (count_code == MFX_E_NOMEM)
      fprintf(stderr, "-- Hint: -passes auto counts the k-mers in passes over key ranges, each in a table of its own that fits -memory and the device.\n");
    return 1;
  }
  mfx_index_info info;
  uint64_t growths = 0;
  if (mfx_index_get_info(ix, &info) || mfx_index_growths(ix, &growths, nullptr, nullptr, nullptr)) DIE_MFX("-count");
  fprintf(stderr, "-- Counted the %d-mers of %lu reads (%lu bases): %lu k-mers, %lu distinct; the table grew %lu time%s to %.3f GB.\n", G.kArg,
          (unsigned long)st.reads, (unsigned long)st.bases, (unsigned long)st.kmers, (unsigned long)info.distinct, (unsigned long)growths,
          growths == 1 ? "" : "s", (double)info.bytes / 1e9);
  const auto tc1 = std::chrono::steady_clock::now();
  uint64_t n = 0;
  if (streamed ? mfx_index_write_db_streamed(ix, 0, G.outName, &n) : mfx_index_write_db(ix, 0, G.outName, &n)) DIE_MFX("-count: writing the database");
  print_wrote(G.outName, n);
  if (env_flag("MFX_CLI_TIMING") > 0)
    fprintf(stderr, "-- count: %.3f s counting, %.3f s sorting and writing\n", std::chrono::duration<double>(tc1 - tc0).count(),
            std::chrono::duration<double>(std::chrono::steady_clock::now() - tc1).count());
  fprintf(stderr, "Bye!\n");
  return 0;
}

// merfin -convert <db> -output <file>: a database in any accepted form rewritten as this program's flat form (sorted
// k-mers in delta-coded blocks), on the host -- no report, no device
static int run_convert(const Globals &G) {
  if (!G.outName) { fprintf(stderr, "No output (-output) supplied.\n"); return 1; }
  fprintf(stderr, "-- Converting '%s' to '%s'.\n", G.convertName, G.outName);
  uint64_t n = 0;
  if (G.placed ? mfx_db_convert_placed(G.convertName, G.outName, &n) : mfx_db_convert(G.convertName, G.outName, &n)) DIE_MFX("-convert");
  print_wrote(G.outName, n);
  fprintf(stderr, "Bye!\n");
  return 0;
}

// merfin -merge a -merge b ... -output <file>: sorted flat databases combined on the GPU window by window (mfx_db_merge); -min / -max act on
// the combined count
static int run_merge(Globals &G) {
  if (!G.devices.empty()) G.device = G.devices[0];
  if (!devices_available({G.device})) return 1;
  static const char *const names[] = {"sum", "max", "min", "intersect"};
  fprintf(stderr, "-- Merging %lu database%s (%s) into '%s'.\n", (unsigned long)G.mergeNames.size(), G.mergeNames.size() == 1 ? "" : "s", names[G.mergeOp], G.outName);
  mfx_db_merge_opts o;
  o.op = G.mergeOp;
  o.minV = G.minV;
  o.maxV = G.maxV;
  o.device = G.device;
  mfx_db_merge_stats st;
  uint64_t subtracted = 0;
  if (G.notNames.empty()) {
    if (mfx_db_merge(G.mergeNames.data(), (uint32_t)G.mergeNames.size(), G.outName, &o, &st)) DIE_MFX("-merge");
  } else {
    fprintf(stderr, "-- Without the k-mers of %lu database%s (-not).\n", (unsigned long)G.notNames.size(), G.notNames.size() == 1 ? "" : "s");
    if (mfx_db_merge_except(G.mergeNames.data(), (uint32_t)G.mergeNames.size(), G.notNames.data(), (uint32_t)G.notNames.size(), G.outName, &o, &st, &subtracted))
      DIE_MFX("-merge -not");
  }
  fprintf(stderr, "-- Merged: %lu k-mers read, %lu written, %lu filtered, %lu saturated, %lu window%s.\n", (unsigned long)st.n_in, (unsigned long)st.n_out,
          (unsigned long)st.n_filtered, (unsigned long)st.n_saturated, (unsigned long)st.windows, st.windows == 1 ? "" : "s");
  if (!G.notNames.empty()) fprintf(stderr, "-- Subtracted: %lu k-mers that a -not database holds.\n", (unsigned long)subtracted);
  print_wrote(G.outName, st.n_out);
  fprintf(stderr, "Bye!\n");
  return 0;
}

// merfin -trio -mat m -pat p [-child c] -output stem: the two hap-mer databases in one windowed pass on the GPU (mfx_db_trio); a cutoff that
// is not given is read off the valley of its k-mer histogram, which is then written beside the databases
static int run_trio(Globals &G) {
  const std::string stem = G.outName, out_a = stem + ".hapA.mfxk", out_b = stem + ".hapB.mfxk";
  fprintf(stderr, "-- Hap-mers of '%s' (A) and '%s' (B)%s%s%s into '%s' and '%s'.\n", G.matName, G.patName, G.childName ? ", kept where '" : "", G.childName ? G.childName : "",
          G.childName ? "' holds them," : "", out_a.c_str(), out_b.c_str());
  mfx_db_trio_opts o;
  o.cut_mat = G.cutMat; o.cut_pat = G.cutPat; o.cut_child = G.childName ? G.cutChild : 0;
  o.max_mult = G.maxMult;
  o.device = G.device;
  const size_t W = (size_t)G.maxMult + 1;
  std::vector<uint64_t> img(3 * W, 0);
  mfx_db_trio_stats st;
  if (mfx_db_trio(G.matName, G.patName, G.childName, out_a.c_str(), out_b.c_str(), &o, img.data(), &st)) DIE_MFX("-trio");
  if (st.hist_pass) {
    static const char *const rows[3] = {".mat_only.hist", ".pat_only.hist", ".child.hist"};
    for (int r = 0; r < (G.childName ? 3 : 2); ++r)
      if (mfx_db_histogram_write(img.data() + r * W, G.maxMult, (stem + rows[r]).c_str())) DIE_MFX("-trio");
  }
  const std::string sname = stem + ".trio.stats";
  FILE *f = fopen(sname.c_str(), "w");
  if (!f) { fprintf(stderr, "ERROR: -trio: cannot open '%s' for writing\n", sname.c_str()); return 1; }
  const std::pair<const char *, unsigned long long> lines[] = {
      {"mat_kmers", st.n_mat}, {"pat_kmers", st.n_pat}, {"child_kmers", st.n_child}, {"both_parents", st.n_both}, {"mat_only", st.n_mat_only}, {"pat_only", st.n_pat_only},
      {"mat_only_at_cutoff", st.n_mat_only_cut}, {"pat_only_at_cutoff", st.n_pat_only_cut}, {"child_at_cutoff", st.n_child_cut}, {"hapA_kmers", st.n_a},
      {"hapB_kmers", st.n_b}, {"windows", st.windows}, {"cut_mat", st.cut_mat}, {"cut_mat_auto", st.auto_mat}, {"cut_pat", st.cut_pat}, {"cut_pat_auto", st.auto_pat},
      {"cut_child", st.cut_child}, {"cut_child_auto", st.auto_child}};
  for (const auto &l : lines) fprintf(f, "%s\t%llu\n", l.first, l.second);
  if (fclose(f) != 0) { fprintf(stderr, "ERROR: -trio: writing '%s' failed\n", sname.c_str()); return 1; }
  fprintf(stderr, "-- Cutoffs: mat %u%s, pat %u%s", st.cut_mat, st.auto_mat ? " (auto)" : "", st.cut_pat, st.auto_pat ? " (auto)" : "");
  if (G.childName) fprintf(stderr, ", child %u%s", st.cut_child, st.auto_child ? " (auto)" : "");
  fprintf(stderr, ".\n-- %lu k-mers of both parents, %lu of mat alone (%lu at the cutoff), %lu of pat alone (%lu), %lu window%s.\n", (unsigned long)st.n_both,
          (unsigned long)st.n_mat_only, (unsigned long)st.n_mat_only_cut, (unsigned long)st.n_pat_only, (unsigned long)st.n_pat_only_cut, (unsigned long)st.windows,
          st.windows == 1 ? "" : "s");
  print_wrote(out_a.c_str(), st.n_a);
  print_wrote(out_b.c_str(), st.n_b);
  fprintf(stderr, "Bye!\n");
  return 0;
}

// merfin -histogram db -output file: `meryl histogram` of a sorted flat database on the GPU (mfx_db_histogram), and what mfx_spectrum_peak reads off it
static int run_histogram(Globals &G) {
  fprintf(stderr, "-- K-mer histogram of '%s' into '%s'.\n", G.histName, G.outName);
  std::vector<uint64_t> row((size_t)G.maxMult + 1, 0);
  uint64_t n = 0;
  if (mfx_db_histogram(G.histName, G.maxMult, row.data(), &n, G.device)) DIE_MFX("-histogram");
  if (mfx_db_histogram_write(row.data(), G.maxMult, G.outName)) DIE_MFX("-histogram");
  mfx_spectrum_peak_t pk;
  const int rc = mfx_spectrum_peak(row.data(), G.maxMult, &pk);
  if (rc == MFX_OK) fprintf(stderr, "-- %lu k-mers; valley %u, main_peak %u, haploid_peak %u.\n", (unsigned long)n, pk.valley, pk.main_peak, pk.haploid_peak);
  else if (rc == MFX_E_NODATA) fprintf(stderr, "-- %lu k-mers; no peak found.\n", (unsigned long)n);
  else DIE_MFX("-histogram");
  fprintf(stderr, "Bye!\n");
  return 0;
}

// ---- the run of a report: what its steps share ------------------------------------------------------------------------------------------
static double epoch() { return std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count(); }

// MFX_CLI_TIMING=1: wall time per phase on stderr at exit (diagnostics; not part of merfin's output); 2: the steps of the index build as well;
// 3: wall-clock stamps (seconds since the epoch) at main / after the device check / at the end, so that a caller who timed the whole process
// can tell start-up and tear-down from the phases
struct PhaseClock {
  typedef std::vector<std::pair<const char *, double>> Marks;
  const int level = env_flag("MFX_CLI_TIMING");
  double stamp_main = 0, stamp_devices = 0;
  std::chrono::steady_clock::time_point t_last, t_sub;
  Marks phases, steps;
  void start(double at_main) { stamp_main = at_main; stamp_devices = epoch(); t_last = t_sub = std::chrono::steady_clock::now(); }
  static void mark(Marks &m, std::chrono::steady_clock::time_point &since, const char *what) {
    const auto t = std::chrono::steady_clock::now();
    m.emplace_back(what, std::chrono::duration<double>(t - since).count());
    since = t;
  }
  void lap(const char *what) { mark(phases, t_last, what); }
  void step(const char *what) { mark(steps, t_sub, what); }
  void print() const {
    if (level <= 0) return;
    fprintf(stderr, "-- timing:");
    for (auto &ph : phases) fprintf(stderr, "  %s %.2fs", ph.first, ph.second);
    fprintf(stderr, "\n");
    if (level > 1 && !steps.empty()) {
      fprintf(stderr, "-- timing (index):");
      for (auto &ph : steps) fprintf(stderr, "  %s %.3fs", ph.first, ph.second);
      fprintf(stderr, "\n");
    }
    if (level > 2) fprintf(stderr, "-- stamps: main %.6f devices %.6f end %.6f\n", stamp_main, stamp_devices, epoch());
  }
};

// sequences (load_Sequence, merfin-globals.C:165-197; loadSequence, merfin.C:30-53).  The file is read (and, for .gz/.bz2/.xz, decompressed) by
// its own thread from start() on; with -seqmers nothing needs the sequence before the evaluation, so the read then runs under the index build
// and is only waited for afterwards (finish()).
struct Sequences {
  std::vector<SeqRecord> recs;
  std::vector<const char *> bases, names;
  std::vector<uint64_t> lens;
  uint64_t totalBases = 0;
  std::thread reader;
  bool readFailed = false;               // written by the reader thread, read after the join
  bool done = false;
  ~Sequences() { if (reader.joinable()) reader.join(); }
  uint32_t size() const { return (uint32_t)recs.size(); }
  bool start(const char *path) {         // false: the file cannot be opened
    auto sf = std::make_shared<SeqFile>(path);
    if (!sf->ok()) return false;
    const std::string seqPath = path;
    reader = std::thread([this, sf, seqPath]() {
      if (read_fasta_parallel(seqPath, recs)) { readFailed = sf->finish() != 0; return; }     // plain FASTA: all host threads
      SeqRecord r;
      while (sf->next(r)) recs.push_back(std::move(r));
      readFailed = sf->finish() != 0;       // a decompressor that died mid-stream: the records read so far are NOT the file
    });
    return true;
  }
  bool finish() {                        // the records are in; false: reading the file failed
    done = true;
    if (reader.joinable()) reader.join();
    if (readFailed) return false;
    bases.resize(recs.size());
    lens.resize(recs.size());
    names.resize(recs.size());
    for (size_t i = 0; i < recs.size(); ++i) { bases[i] = recs[i].data(); lens[i] = recs[i].size(); names[i] = recs[i].name.c_str(); totalBases += lens[i]; }
    return true;
  }
};

struct Run {
  Globals &G;
  int k = 0;
  mfx_db_info rdb, adb;
  const bool fromReads, variantMode;
  const bool fullIndex = env_flag("MFX_CLI_FULL_INDEX") > 0;     // the full tables for every report type
  const int vcfAheadKnob = env_flag("MFX_CLI_VCF_AHEAD");
  bool seqOnly = false;                  // -hist, -dump, -track: the sequence-only index (decide_seq_only_and_defer)
  bool pathOnly = false;                 // the variant modes on the path-only index of their call set (decide_path_only)
  bool streamHist = false, deferSeq = false;
  uint64_t basesBound = 0, fingerprint = 0, fingerprintFull = 0;
  PhaseClock clock;
  mfx_kparams kp;
  Owned<mfx_db_stage, mfx_db_stage_free> stage, stageAsm;        // (stageAsm: -seqmers of the path-only index)
  Owned<mfx_index, mfx_index_free> ix;
  Owned<mfx_seq, mfx_seq_free> seq;
  Owned<mfx_eval, mfx_eval_free> ev;
  Sequences S;
  std::string vcfAheadError;
  Owned<mfx_vcf, mfx_vcf_free> vcfReady;                         // the call set taken from vcfLoad (prepared): report_variants uses it
  VcfFuture vcfLoad, vcfAhead;                                   // (last: their threads read the members above)
  explicit Run(Globals &g) : G(g), fromReads(!g.readsNames.empty()), variantMode(variant_mode(g.reportType)) {}
};

static size_t variant_slots(const Globals &G) {
  const int vs = env_flag("MFX_VARIANT_SLOTS");
  return vs > 0 ? (size_t)vs : G.devices.size();
}

// load_Kmers, merfin-globals.C:114-163: the read DB defines k
static int probe_databases(Run &R) {
  const Globals &G = R.G;
  memset(&R.rdb, 0, sizeof(R.rdb));
  if (!R.fromReads && mfx_db_probe(G.readDBname, &R.rdb)) DIE_MFX("opening -readmers");
  R.k = R.fromReads ? G.kArg : R.rdb.k;                           // (-reads: -k, or the k of -seqmers, checked before)
  memset(&R.adb, 0, sizeof(R.adb));
  if (G.seqDBname) {
    if (mfx_db_probe(G.seqDBname, &R.adb)) DIE_MFX("opening -seqmers");
    if (R.adb.k != R.k) { fprintf(stderr, "ERROR: -seqmers holds %d-mers but -readmers holds %d-mers.\n", R.adb.k, R.k); return 1; }
  }
  if (R.rdb.format == MFX_DB_MERYL || (G.seqDBname && R.adb.format == MFX_DB_MERYL))
    fprintf(stderr, "-- NOTE: meryl database directories are decoded from a recalled description of the format; it has not been\n"
                    "--       checked against upstream meryl.  The decoder cross-checks every database against its own index\n"
                    "--       statistics; `meryl print` text is the verified interchange form.  To validate the decoder on this\n"
                    "--       database: python tools/meryl_conformance.py <db.meryl> <output of `meryl print db.meryl`>\n"
                    "--       (= MFX_REAL_MERYL_DB / MFX_REAL_MERYL_PRINT for tests/test_gpu_meryl_conformance.py).\n");
  return 0;
}

// `merfin -hist / -dump -sequence s -readmers db` on one device with a delta-coded database and no -seqmers: the database's bytes start
// moving into device memory NOW, on a thread of their own (mfx_db_stage_begin) -- under the FASTA read, the sequence upload, the
// table's allocation and the kernel that claims the sequence's k-mers.  Any other database form, too little free memory,
// MFX_DB_STAGE=0: no stage, the build reads the database when it gets there.
static void begin_stage(Run &R) {
  const Globals &G = R.G;
  const bool histLike = (G.reportType == OP_HIST || G.reportType == OP_DUMP || G.reportType == OP_TRACK || G.reportType == OP_REGIONS) && !G.sharded && R.k <= 31 && G.seqName && !G.seqDBname &&
                        !G.indexName && G.devices.size() == 1 && !R.fullIndex;
  if (histLike && R.rdb.format == MFX_DB_FLAT) R.stage = mfx_db_stage_begin(G.readDBname, G.device);
}
// the path-only index of the variant modes: both databases move while the call set is prepared and its paths are claimed -- from the moment
// the sequences are in (under the FASTA reader the stagers' threads cost it 0.2 s of a 3 Gb file on a 16-core quota)
static void begin_path_stages(Run &R) {
  const Globals &G = R.G;
  if (R.rdb.format == MFX_DB_FLAT) R.stage = mfx_db_stage_begin(G.readDBname, G.device);
  if (G.seqDBname && R.adb.format == MFX_DB_FLAT) R.stageAsm = mfx_db_stage_begin(G.seqDBname, G.device);
}

// The variant modes ask the lookup tables for the k-mers of the enumerated PATHS and nothing else (varMer::score, varMer.C:76-84): one slot
// on one device can prepare the call set first (host work), claim exactly those k-mers on a sequence-only index while it does
// (mfx_vcf_prepare_path_index) and let both databases update them -- the PATH-ONLY index, a thirteenth of the full tables (3 Gb, 3.7 M calls:
// 10.3 GB instead of 137; device work of the build 0.27 instead of 0.65 s).  Its price is the order: the VCF and the clusters' paths come
// BEFORE the index instead of under its build -- on a 16-core host 1.9-2.1 s against 1.55-1.65 s of wall (profiles/r06_cfg4_cli.txt).  So it
// is what a run takes when the full tables do not fit (-memory, or 90 % of the device's free memory), and MFX_CLI_PATH_INDEX=1 / 0 says
// so explicitly.  Not with -index (the image caches the full tables), k > 31, several slots, MFX_CLI_VCF_AHEAD=0.
static int decide_path_only(Run &R) {
  const Globals &G = R.G;
  const int pe = env_flag("MFX_CLI_PATH_INDEX");
  const bool can = R.variantMode && G.vcfName && G.seqName && variant_slots(G) == 1 && !G.sharded && R.k <= 31 && !G.indexName &&
                   (R.fromReads || (R.vcfAheadKnob != 0 && !R.fullIndex));
  if (R.fromReads && R.variantMode) {
    // (the reads are counted into the k-mers the call set's paths ask for: there is no read database for the full tables)
    if (!can) { fprintf(stderr, "ERROR: the variant modes count -reads into the path-only index of the call set, which this run cannot take.\n"); return 1; }
    R.pathOnly = true;
  } else if (can && pe >= 0) R.pathOnly = pe != 0;
  else if (can) {
    const uint64_t capacity = R.rdb.n_kmers + (G.seqDBname ? R.adb.n_kmers : bases_upper_bound(G.seqName)) + 1024;
    const double fullGB = mfx_index_estimate_gb(R.k, capacity);
    uint64_t freeB = 0, totalB = 0;
    const bool known = mfx_device_memory(G.device, &freeB, &totalB) == MFX_OK;
    R.pathOnly = (G.maxMemory > 0 && fullGB > G.maxMemory) || (known && fullGB * 1e9 > 0.9 * (double)freeB);
    if (R.pathOnly)
      fprintf(stderr, "-- The full lookup tables would take %.1f GB (%s %.1f GB): building the path-only index of the call set instead.\n", fullGB,
              G.maxMemory > 0 && fullGB > G.maxMemory ? "-memory allows" : "free on the device:", G.maxMemory > 0 && fullGB > G.maxMemory ? G.maxMemory : freeB / 1e9);
  }
  // the path-only index is built FROM the call set: its VCF is read and parsed (host work only) while the FASTA file is
  if (R.pathOnly)
    R.vcfLoad.f = std::async(std::launch::async, [&R]() {
      mfx_vcf *v = mfx_vcf_load(R.G.vcfName);
      if (!v) R.vcfAheadError = mfx_last_error();                  // (errors are per thread: carried to the caller's)
      return v;
    });
  return 0;
}

// -hist and -dump ask the lookup tables for the k-mers of -sequence and nothing else (merfin-histogram.C:54-64,
// merfin-dump.C:44-61): they get a SEQUENCE-ONLY index -- the sequence's k-mers are claimed first, the databases only
// update those (half of a 30x human read database, the error k-mers, never gets a slot; k <= 21: 8-byte slots).  The
// other report types need the whole read database.  MFX_CLI_FULL_INDEX=1 builds the full tables for every type.
// (-reads: always -- the reads are counted into claimed k-mers; there is no read database for the full tables)
// (-spectrum: the full tables from -readmers -- its read-only row needs every read k-mer; with -reads the index -hist would build)
// deferSeq: with -seqmers, and without it whenever the file tells an upper bound of its bases -- the table is sized by the bound, the
// read database is loaded while the file is read, the assembly k-mers are counted once it is in.
// Only compressed files are worth it: their decompression takes seconds per Gb on one core, while a plain file is parsed
// at 2-5 GB/s and reading it under the build measurably slows the build's own readers (1 Gb: 1.8-3.0 s read first,
// 2.4-3.2 s overlapped; MFX_CLI_OVERLAP=1 / 0 forces either).
static void decide_seq_only_and_defer(Run &R, bool compressed) {
  const Globals &G = R.G;
  R.seqOnly = (G.reportType == OP_HIST || G.reportType == OP_DUMP || G.reportType == OP_TRACK || G.reportType == OP_REGIONS || (G.reportType == OP_SPECTRUM && R.fromReads)) && !G.sharded &&
              R.k <= 31 && (R.fromReads || !R.fullIndex);
  const int ov = env_flag("MFX_CLI_OVERLAP");
  const bool wantOverlap = ov >= 0 ? ov != 0 : compressed;
  R.basesBound = (G.seqName && !G.seqDBname && wantOverlap && !R.seqOnly) ? bases_upper_bound(G.seqName) : 0;
  R.deferSeq = G.seqName && !G.sharded && !R.seqOnly && !R.pathOnly && wantOverlap && (G.seqDBname || R.basesBound > 0);   // (the path-only index needs the sequences first)
}

// the reader thread is joined, the records are in.  1: reading failed (the error is printed)
static int finish_seq(Run &R) {
  if (R.S.done) return 0;
  if (!R.S.finish()) {
    fprintf(stderr, "ERROR: reading '%s' failed (read error, or the decompressor exited with an error: truncated or corrupt file?).\n", R.G.seqName);
    return 1;
  }
  R.clock.lap("read sequences");
  return 0;
}

// the sequences to the device.  -hist on one device with the assembly k-mers coming from -seqmers (streamHist): nothing needs the sequence in
// HBM before the evaluation, so its upload is streamed under the -hist kernel (mfx_hist_run_streamed).  Otherwise the index build
// counts the assembly k-mers from the packed sequence and it goes up first.  false: mfx_last_error says why
static bool make_seq(Run &R) {
  const Globals &G = R.G;
  if (!R.S.recs.empty() || G.seqName) {
    R.seq = R.streamHist ? mfx_seq_create(G.device, R.S.lens.data(), R.S.size()) : mfx_seq_upload(G.device, R.S.bases.data(), R.S.lens.data(), R.S.size());
    if (!R.seq) return false;
  }
  R.clock.lap("upload sequences");
  if (R.stage) mfx_db_stage_boost(R.stage);                       // the host's threads are free: the database's readers may have them all
  return true;
}

// -sharded: -hist / -dump take a part of the sequences per device, each on the sequence-only index of ITS k-mers (no exchange);
// everything else -- and a non-canonical database -- takes the hash-sharded full tables (MFX_CLI_FULL_INDEX=1: always)
static int run_on_shards(Run &R) {
  const Globals &G = R.G;
  if (G.devices.size() < 2) { fprintf(stderr, "ERROR: -sharded needs at least two -devices.\n"); return 1; }
  if (G.indexName) { fprintf(stderr, "ERROR: -index caches a whole table; it cannot be combined with -sharded.\n"); return 1; }
  if ((G.reportType == OP_HIST || G.reportType == OP_DUMP) && R.k <= 31 && !R.fullIndex) {
    const int prc = run_parts(G, R.k, R.S.recs, R.S.bases, R.S.lens);
    if (prc >= 0) return prc;
  }
  return run_sharded(G, R.k, R.rdb, R.adb, R.S.recs, R.S.bases, R.S.lens, R.S.names, R.S.totalBases);
}

// variant modes on one slot: the VCF is read and parsed (host work only) on a thread of its own while the index is built
// (merfin opens it after load_Kmers, merfin-globals.C:201-219; 0.15 s of a 4 M-call set).  An error is reported where the
// VCF is opened (report_variants).  Several slots split the file per slot instead.
static void start_vcf_ahead(Run &R) {
  const Globals &G = R.G;
  if (!(R.variantMode && G.vcfName && variant_slots(G) == 1 && !G.sharded && R.vcfAheadKnob != 0 && !R.pathOnly)) return;
  R.vcfAhead.f = std::async(std::launch::async, [&R]() {
    const Globals &G = R.G;
    mfx_vcf *v = mfx_vcf_load(G.vcfName);
    if (!v) { R.vcfAheadError = mfx_last_error(); return v; }    // (errors are per thread: carried to the caller's)
    // MFX_CLI_VCF_AHEAD=2: ... and its clusters merged, their allele combinations enumerated and packed here as well (mfx_vcf_prepare:
    // stage A of the run needs the sequences, not the index).  Not the default: on a host whose cores the index build already
    // keeps busy (the 16-core quota of the measured boxes: its readers copy 13 GB out of the page cache) the two slow each other
    // down -- config 4 at 3 Gb 2.02-2.07 s with the load alone ahead, 2.67-2.75 s with stage A too (profiles/r05_cfg4_cli_ahead.txt).
    // (never while the sequences are still being read -- deferSeq: finish_seq() fills recs / bases / lens on the main thread later)
    if (R.vcfAheadKnob != 2 || R.deferSeq) return v;
    const mfx_variant_opts o = variant_opts(G, G.debug ? "-" : nullptr);
    if (mfx_vcf_prepare(v, R.k, R.S.names.data(), R.S.bases.data(), R.S.lens.data(), R.S.size(), &o)) {
      R.vcfAheadError = mfx_last_error();
      mfx_vcf_free(v);
      v = nullptr;
    }
    return v;
  });
}

// ---- the index: an image of it, or one of three builds ------------------------------------------------------------------------------------
static void memory_banner(const Globals &G, double neededGB, const std::string &of_what = "") {
  fprintf(stderr, "--\n-- Memory needed: %.3f GB%s\n-- Memory limit:  %.3f GB%s\n--\n", neededGB, of_what.c_str(), G.maxMemory, G.maxMemory > 0 ? "" : " (none)");
}

// A database into the table (side 1: -seqmers, 0: -readmers with -min / -max), from its stage when it has one.  Returns 0, or `tolerated`
// for the caller to fall back on, or 1 with the error printed.  label: the step of the phase clock this was
static int load_db_step(Run &R, const char *path, int side, mfx_db_stage *stage, const char *label, int tolerated = MFX_E_NONCANON) {
  const uint64_t lo = side ? 0 : R.G.minV, hi = side ? ~0ull : R.G.maxV;
  fprintf(stderr, "-- Loading kmers from '%s' into lookup table.\n", path);
  const int lrc = stage ? mfx_index_load_db_staged(R.ix, stage, side, lo, hi) : mfx_index_load_db(R.ix, path, side, lo, hi);
  if (lrc && lrc != tolerated) DIE_MFX(side ? "loading -seqmers" : "loading -readmers");
  if (label) R.clock.step(label);
  return lrc;
}

static int save_index_image(Run &R) {
  fprintf(stderr, "-- Writing the index image '%s'.\n", R.G.indexName);
  if (mfx_index_set_fingerprint(R.ix, R.fingerprint) || mfx_index_save(R.ix, R.G.indexName)) DIE_MFX("writing the index image");
  return 0;
}

// -index: the image is loaded if it exists and was built from these inputs; R.ix stays empty when the run has to build
static int load_index_image(Run &R) {
  const Globals &G = R.G;
  FILE *probe = G.indexName ? fopen(G.indexName, "rb") : nullptr;
  R.fingerprint = G.indexName ? input_fingerprint(G, R.seqOnly) : 0;
  // a run that would build the sequence-only index also accepts a FULL image of the same inputs: that is what such a run
  // saved when a database turned out not to be canonical (the fallback of main) -- without this every later run would
  // build twice again and the cache would never take effect
  R.fingerprintFull = (G.indexName && R.seqOnly) ? input_fingerprint(G, false) : R.fingerprint;
  if (!probe) return 0;
  fclose(probe);
  fprintf(stderr, "-- Loading the index image '%s' (k-mer databases are not read).\n", G.indexName);
  R.ix = mfx_index_load(G.indexName, G.maxMemory, G.device);
  if (!R.ix) { fprintf(stderr, "\n%s\n\n", mfx_last_error()); return 1; }
  mfx_index_info info;
  if (mfx_index_get_info(R.ix, &info)) DIE_MFX("reading the index image");
  if (info.k != R.k) { fprintf(stderr, "ERROR: the index image holds %d-mers but %s %d-mers.\n", info.k, R.fromReads ? "the run counts" : "-readmers holds", R.k); return 1; }
  uint64_t fp = 0, imin = 0, imax = 0;
  if (mfx_index_get_origin(R.ix, &fp, &imin, &imax)) DIE_MFX("reading the index image");
  if (R.seqOnly && info.seq_only == 0 && fp == R.fingerprintFull && imin == G.minV && imax == G.maxV) {
    R.seqOnly = false;                                              // the full tables of these inputs (a non-canonical database)
    R.fingerprint = R.fingerprintFull;
  } else if (fp != R.fingerprint || imin != G.minV || imax != G.maxV || (info.seq_only != 0) != R.seqOnly) {
    // the image was built from other inputs (a re-polished -sequence, another database, other -min/-max):
    // using it would give wrong asmK / readK with no diagnostic
    fprintf(stderr, "-- The index image '%s' was built from other inputs (%s); rebuilding it.\n", G.indexName,
            (imin != G.minV || imax != G.maxV) ? "-min/-max differ" : "a database or the sequence file changed");
    R.ix.reset();
  }
  return 0;
}

// The three builds return 0 with R.ix built, 1 with the error printed, or -1: this index cannot be had, build the full tables.

// The PATH-ONLY index of the variant modes, from the call set that vcfLoad read
static int build_path_only_index(Run &R) {
  const Globals &G = R.G;
  R.vcfReady = R.vcfLoad.f.get();
  if (!R.vcfReady) { fprintf(stderr, "ERROR: variant scoring: %s\n", R.vcfAheadError.c_str()); return 1; }
  R.clock.step("(before the index: sequences, VCF)");
  // the clusters merged, the table made from the bound of their path text, then batch by batch: the paths' tables packed on the host, their
  // k-mers claimed on the device under the next batch's packing (mfx_vcf_prepare_path_index)
  fprintf(stderr, "-- Claiming the %d-mers of the variants' paths on the GPU.\n", R.k);
  const mfx_variant_opts o = variant_opts(G, G.debug ? "-" : nullptr);
  mfx_index *claimed = nullptr;
  if (mfx_vcf_prepare_path_index(R.vcfReady, R.k, R.S.names.data(), R.S.bases.data(), R.S.lens.data(), R.S.size(), &o, G.maxMemory, G.device, 0.7, &claimed))
    DIE_MFX("preparing the call set");
  R.ix = claimed;
  if (!R.ix) fprintf(stderr, "-- %s\n-- Building the full lookup tables instead.\n", mfx_last_error());
  if (R.ix) {
    mfx_index_info info;
    if (mfx_index_get_info(R.ix, &info)) DIE_MFX("reading the path-only index");
    memory_banner(G, info.bytes / 1e9, " (the " + std::to_string(R.k) + "-mers of the variants' paths: " + std::to_string(info.distinct) + ")");
  }
  if (R.stage) mfx_db_stage_boost(R.stage);                         // the host's threads are free: the databases' readers may have them all
  if (R.stageAsm) mfx_db_stage_boost(R.stageAsm);
  R.clock.step("prepare the call set + claim the paths' k-mers");
  int lrc = 0;
  if (R.ix) {
    if (G.seqDBname) {
      lrc = load_db_step(R, G.seqDBname, 1, R.stageAsm, "load -seqmers");
      if (lrc == 1) return 1;
      R.stageAsm.reset();
    } else {
      // replaces `meryl count k=.. <seq> output <seq>.meryl` (merfin-globals.C:182-186) for the k-mers that will be asked for
      fprintf(stderr, "-- No -seqmer given. Counting the %d-mers of '%s' on the GPU.\n", R.k, G.seqName);
      if (!R.seq && !make_seq(R)) DIE_MFX("uploading sequences");
      if (mfx_index_count_claimed(R.ix, R.seq, nullptr)) DIE_MFX("counting sequence k-mers");
      R.clock.step("count the sequence's k-mers");
    }
    if (!lrc && R.fromReads) {
      if (!count_reads_files(G, R.ix)) return 1;
      R.clock.step("count -reads");
    } else if (!lrc) {
      lrc = load_db_step(R, G.readDBname, 0, R.stage, "load -readmers");
      if (lrc == 1) return 1;
    }
    if (lrc == MFX_E_NONCANON) {
      fprintf(stderr, "-- A k-mer database is not canonical; building the full lookup tables instead.\n");
      R.ix.reset();
    }
  }
  // (the staged bytes are not needed by the run; a fall-back to the full tables reads the files)
  R.stage.reset();
  R.stageAsm.reset();
  if (!R.ix && R.fromReads) { fprintf(stderr, "ERROR: -reads needs the path-only index of the call set, which could not be built.\n"); return 1; }
  return R.ix ? 0 : -1;
}

// The SEQUENCE-ONLY index of -hist, -dump and -track
static int build_seq_only_index(Run &R) {
  const Globals &G = R.G;
  const uint64_t capacity = R.S.totalBases + 1024;                // a sequence has at most one new k-mer per base
  memory_banner(G, mfx_index_estimate_gb_for_seq(R.k, capacity));
  R.clock.step("(before the index)");
  // load factor of the table: 0.4 unless the user says otherwise (MFX_LOAD_FACTOR) -- the emptier tables the library would pick probe
  // faster (3 Gb: 20 instead of 23 ms of -hist kernel) but a run that starts behind another waits seconds in hipMalloc for the driver
  // to clear what that one freed, the longer the more of the HBM both ask for (profiles/r05_e2e_lf_ab.txt)
  R.ix = mfx_index_create_for_seq_lf(R.k, capacity, G.maxMemory, G.device, 0.4);
  if (!R.ix && R.stage) {                                           // (the staged database may be what the table lacks)
    R.stage.reset();
    R.ix = mfx_index_create_for_seq_lf(R.k, capacity, G.maxMemory, G.device, 0.4);
  }
  if (!R.ix) { fprintf(stderr, "\n%s\n\n", mfx_last_error()); return 1; }
  R.clock.step("create the table");
  int lrc = 0;
  bool fused = false;
  if (G.seqDBname) {
    fprintf(stderr, "-- Claiming the %d-mers of '%s' on the GPU.\n", R.k, G.seqName);
    if (mfx_index_claim_seq(R.ix, R.seq, nullptr)) DIE_MFX("claiming sequence k-mers");
    R.clock.step("claim the sequence's k-mers");
    lrc = load_db_step(R, G.seqDBname, 1, nullptr, "load -seqmers");
    if (lrc == 1) return 1;
  } else if (R.fromReads) {
    fprintf(stderr, "-- No -seqmer given. Counting the %d-mers of '%s' on the GPU.\n", R.k, G.seqName);
    if (mfx_index_count_asm(R.ix, R.seq, nullptr)) DIE_MFX("counting sequence k-mers");
    R.clock.step("count the sequence's k-mers");
  } else {
    // replaces `meryl count k=.. <seq> output <seq>.meryl` (merfin-globals.C:182-186)
    // (this build says "No -seqmer given" before "Loading kmers", the full tables the other way round: each follows the order of its own calls)
    fprintf(stderr, "-- No -seqmer given. Counting the %d-mers of '%s' on the GPU.\n", R.k, G.seqName);
    // (one call for the counting and the load of -readmers: the database crosses PCIe while the k-mers are claimed)
    fprintf(stderr, "-- Loading kmers from '%s' into lookup table.\n", G.readDBname);
    lrc = R.stage ? mfx_index_build_for_hist_staged(R.ix, R.seq, R.stage, G.minV, G.maxV) : mfx_index_build_for_hist(R.ix, R.seq, G.readDBname, G.minV, G.maxV);
    R.stage.reset();                                                // its device memory is not needed by the evaluation
    if (lrc && lrc != MFX_E_NONCANON) DIE_MFX("counting sequence k-mers / loading -readmers");
    R.clock.step("count the sequence's k-mers + load -readmers");
    fused = true;
  }
  if (lrc == MFX_E_NONCANON && R.fromReads) { fprintf(stderr, "ERROR: -reads needs a canonical -seqmers database.\n"); return 1; }
  if (!lrc && R.fromReads) {
    if (!count_reads_files(G, R.ix)) return 1;
    R.clock.step("count -reads");
  } else if (!lrc && !fused) {
    lrc = load_db_step(R, G.readDBname, 0, nullptr, "load -readmers");
    if (lrc == 1) return 1;
  }
  if (lrc == MFX_E_NONCANON) {
    // one slot per canonical k-mer cannot answer value(fmer) + value(rmer) of a non-canonical database
    fprintf(stderr, "-- A k-mer database is not canonical; building the full lookup tables instead.\n");
    R.ix.reset();
    return -1;
  }
  return G.indexName ? save_index_image(R) : 0;
}

// The full lookup tables.  The table is sized before the sequence is in when the file promised a bound on its bases; a file that breaks the
// promise (several gzip members, ...) costs a second build with the true number
static int build_full_index(Run &R) {
  const Globals &G = R.G;
  for (int attempt = 0; !R.ix; ++attempt) {
    const uint64_t capacity = R.rdb.n_kmers + (G.seqDBname ? R.adb.n_kmers : (R.S.done ? R.S.totalBases : R.basesBound)) + 1024;
    memory_banner(G, mfx_index_estimate_gb(R.k, capacity));
    // (the smallest table the library makes, load factor 0.7: the device stage of these report types is a hundredth of the run, and a
    // table allocated behind another process waits for the driver to clear what that one freed -- the longer, the larger both are)
    R.ix = mfx_index_create_lf(R.k, capacity, G.maxMemory, G.device, 0.7);
    if (!R.ix && !G.seqDBname && !R.S.done && R.basesBound > 0) {
      // the capacity came from the file's BOUND on its bases (a .gz of a human assembly sits near the 4 GiB step of that
      // bound): read the file to the end, as the reference does before anything else, and size the table by the truth
      fprintf(stderr, "-- The table sized by the bound on the bases of '%s' does not fit; reading the file first.\n", G.seqName);
      if (finish_seq(R)) return 1;
      continue;
    }
    if (!R.ix) {
      const bool nomem = mfx_last_error_code() == MFX_E_NOMEM;
      fprintf(stderr, "\n%s\n\n", mfx_last_error());
      if (nomem && (G.reportType == OP_COMPL || G.reportType == OP_SPECTRUM) && !R.fromReads && G.seqDBname && R.rdb.format == MFX_DB_FLAT && !R.rdb.placed &&
          R.adb.format == MFX_DB_FLAT && !R.adb.placed)
        fprintf(stderr, "-- Hint: -join runs this report from the two sorted databases window by window, without a table: neither has to fit the device.\n");
      return 1;
    }
    if (!R.fromReads && load_db_step(R, G.readDBname, 0, nullptr, nullptr, 0)) return 1;
    if (G.seqDBname) {
      if (load_db_step(R, G.seqDBname, 1, nullptr, nullptr, 0)) return 1;
      break;
    }
    // replaces `meryl count k=.. <seq> output <seq>.meryl` (merfin-globals.C:182-186)
    if (R.deferSeq && !R.S.done) {            // the read database is in; now the sequence is needed
      if (finish_seq(R)) return 1;
      if (R.S.totalBases > R.basesBound && attempt == 0) {
        fprintf(stderr, "-- NOTE: '%s' holds %lu bases, more than its size promised (%lu); rebuilding the table.\n", G.seqName,
                (unsigned long)R.S.totalBases, (unsigned long)R.basesBound);
        R.ix.reset();
        continue;
      }
    }
    if (!R.seq && !make_seq(R)) DIE_MFX("uploading sequences");
    fprintf(stderr, "-- No -seqmer given. Counting the %d-mers of '%s' on the GPU.\n", R.k, G.seqName);
    if (mfx_index_count_asm(R.ix, R.seq, nullptr)) DIE_MFX("counting sequence k-mers");
  }
  // -reads (k > 31: this table holds the assembly's k-mers only; the reads update them)
  if (R.fromReads && !count_reads_files(G, R.ix)) return 1;
  return G.indexName ? save_index_image(R) : 0;
}

// ---- the reports ---------------------------------------------------------------------------------------------------------------------------
// -spectrum / -peak auto: one streaming pass over the table (mfx_spectrum_run), the haploid peak off its single-copy row
// the spectrum's file and what stderr says of it: shared by the table route and -join
static int write_spectrum_report(const Globals &G, int k, const std::vector<uint64_t> &img, uint64_t entries, bool withReadOnly) {
  const uint32_t copies = G.copies, maxMult = G.maxMult;
  const std::string name = std::string(G.outName) + ".spectra-cn.hist";
  fprintf(stderr, "-- Copy-number spectrum of the %d-mers to '%s'.\n", k, name.c_str());
  if (mfx_spectrum_write(img.data(), copies, maxMult, withReadOnly ? 1 : 0, name.c_str())) DIE_MFX("writing the spectrum");
  uint64_t asmOnly = 0, readOnly = 0;
  for (uint32_t r = 1; r < copies + 2; ++r) asmOnly += img[(size_t)r * (maxMult + 1)];
  for (uint32_t m = 0; m <= maxMult; ++m) readOnly += img[m];
  fprintf(stderr, "Entries counted: %lu\nAssembly-only k-mers: %lu\n", (unsigned long)entries, (unsigned long)asmOnly);
  if (withReadOnly) fprintf(stderr, "Read-only k-mers: %lu\n", (unsigned long)readOnly);
  else fprintf(stderr, "The table holds the k-mers of -sequence only (-reads): the read-only row is left out.\n");
  return 0;
}

static int run_spectrum_or_peak(Run &R) {
  Globals &G = R.G;
  const bool report = G.reportType == OP_SPECTRUM;
  const uint32_t copies = report ? G.copies : 4u, maxMult = report ? G.maxMult : 10000u;
  std::vector<uint64_t> img((size_t)(copies + 2) * (maxMult + 1));
  uint64_t entries = 0;
  if (mfx_spectrum_run(R.ix, copies, maxMult, img.data(), &entries)) DIE_MFX(report ? "-spectrum" : "-peak auto");
  // a table that holds the k-mers of -sequence only (-reads) has no read-only k-mers: the row is left out, not written as zeros
  if (report && write_spectrum_report(G, R.k, img, entries, !R.fromReads)) return 1;
  mfx_spectrum_peak_t pk;
  if (mfx_spectrum_peak(img.data() + (size_t)(maxMult + 1), maxMult, &pk) == MFX_OK) {
    fprintf(stderr, "Haploid peak (auto): %u  (main peak %u, valley %u, single-copy k-mers at the peak %lu)\n", pk.haploid_peak, pk.main_peak, pk.valley,
            (unsigned long)pk.count_at_peak);
    if (G.peakAuto) G.peak = (double)pk.haploid_peak;
  } else if (report) {
    fprintf(stderr, "No haploid peak found in the single-copy row (%s); the other report types need -peak <number>.\n", mfx_last_error());
  } else {
    fprintf(stderr, "ERROR: -peak auto found no haploid peak in the single-copy row of the spectrum (%s). Give -peak <number>.\n", mfx_last_error());
    return 1;
  }
  R.clock.lap("spectrum");
  return 0;
}

// merfin -completeness -join / -spectrum -join: the report from the sorted join of -readmers and -seqmers (mfx_db_join_*), no table.  The
// texts are the table route's.
static int run_join(const Globals &G) {
  mfx_db_join_opts o;
  memset(&o, 0, sizeof(o));
  o.device = G.device;
  o.minV = G.minV; o.maxV = G.maxV;
  o.peak = G.peak;
  o.n_prob = (uint32_t)G.copyKmerK.size(); o.probK = G.copyKmerK.data(); o.probP = G.copyKmerP.data();
  o.copies = G.copies; o.max_mult = G.maxMult;
  mfx_db_join_stats st;
  fprintf(stderr, "-- Joining '%s' and '%s' window by window.\n", G.readDBname, G.seqDBname);
  if (G.reportType == OP_COMPL) {
    fprintf(stderr, "-- Compute completeness.\n");
    double t64[64], u64[64];
    if (mfx_db_join_completeness(G.readDBname, G.seqDBname, &o, t64, u64, &st)) DIE_MFX("-completeness -join");
    print_completeness(t64, u64);
  } else {
    mfx_db_info rdb;
    if (mfx_db_probe(G.readDBname, &rdb)) DIE_MFX("opening -readmers");
    std::vector<uint64_t> img((size_t)(G.copies + 2) * (G.maxMult + 1));
    uint64_t entries = 0;
    if (mfx_db_join_spectrum(G.readDBname, G.seqDBname, &o, img.data(), &entries, &st)) DIE_MFX("-spectrum -join");
    if (write_spectrum_report(G, rdb.k, img, entries, true)) return 1;
    mfx_spectrum_peak_t pk;
    if (mfx_spectrum_peak(img.data() + (size_t)(G.maxMult + 1), G.maxMult, &pk) == MFX_OK)
      fprintf(stderr, "Haploid peak (auto): %u  (main peak %u, valley %u, single-copy k-mers at the peak %lu)\n", pk.haploid_peak, pk.main_peak, pk.valley,
              (unsigned long)pk.count_at_peak);
    else fprintf(stderr, "No haploid peak found in the single-copy row (%s); the other report types need -peak <number>.\n", mfx_last_error());
  }
  fprintf(stderr, "-- Joined: %lu read k-mers, %lu assembly k-mers, %lu in both, %lu window%s.\n", (unsigned long)st.n_read, (unsigned long)st.n_asm,
          (unsigned long)st.n_both, (unsigned long)st.windows, st.windows == 1 ? "" : "s");
  fprintf(stderr, "Bye!\n");
  return 0;
}

// merfin -diploid -readmers r -hap1 a -hap2 b -output stem: two haplotype assemblies against the reads in one join (mfx_db_diploid), no table.
// The QV is mfx_histoQV over the assembly's k-mers the reads do not hold; it and the completeness follow Merqury's in spirit and are not
// validated against Merqury.
static bool write_diploid_text(const std::string &name, const std::string &text) {
  FILE *f = fopen(name.c_str(), "w");
  if (!f) { fprintf(stderr, "ERROR: -diploid: cannot open '%s' for writing\n", name.c_str()); return false; }
  const bool ok = fputs(text.c_str(), f) >= 0;
  if (fclose(f) != 0 || !ok) { fprintf(stderr, "ERROR: -diploid: writing '%s' failed\n", name.c_str()); return false; }
  return true;
}

static int run_diploid(Globals &G) {
  const char *h1 = G.hap1Names[0], *h2 = G.hap2Names[0];
  mfx_db_join_opts o;
  memset(&o, 0, sizeof(o));
  o.device = G.device;
  o.minV = G.minV; o.maxV = G.maxV;
  o.peak = G.peak;
  o.n_prob = (uint32_t)G.copyKmerK.size(); o.probK = G.copyKmerK.data(); o.probP = G.copyKmerP.data();
  o.copies = G.copies; o.max_mult = G.maxMult;
  mfx_db_info rdb;
  if (mfx_db_probe(G.readDBname, &rdb)) DIE_MFX("opening -readmers");
  const size_t W = (size_t)G.maxMult + 1;
  std::vector<uint64_t> cls(4 * W), cn((size_t)(G.copies + 2) * W);
  uint64_t entries = 0;
  mfx_db_diploid_stats st;
  double t64[64], u64[3 * 64];
  const bool peak = G.peakGiven;
  fprintf(stderr, "-- Joining '%s' with '%s' and '%s' window by window.\n", G.readDBname, h1, h2);
  if (mfx_db_diploid(G.readDBname, h1, h2, &o, cls.data(), cn.data(), &entries, &st, peak ? t64 : nullptr, peak ? u64 : nullptr)) DIE_MFX("-diploid");
  const std::string stem = G.outName;
  fprintf(stderr, "-- Spectrum of the %d-mers by assembly to '%s'.\n", rdb.k, (stem + ".spectra-asm.hist").c_str());
  if (mfx_diploid_write_asm(cls.data(), G.maxMult, (stem + ".spectra-asm.hist").c_str())) DIE_MFX("writing the spectrum");
  if (write_spectrum_report(G, rdb.k, cn, entries, true)) return 1;
  const char *const names[3] = {"hap1", "hap2", "both"};
  const mfx_diploid_counts *const x[3] = {&st.hap1, &st.hap2, &st.both};
  char line[512];
  std::string qv = "# QV = -10 log10(1 - (1 - only / all)^(1 / k)): Merqury's in spirit, unvalidated against Merqury\n#name\tonly_total\ttotal\tQV\terror\n";
  for (int pass = 0; pass < 2; ++pass) {
    if (pass) qv += "#name\tonly_distinct\tdistinct\tQV\terror\n";
    for (int i = 0; i < 3; ++i) {
      const uint64_t only = pass ? x[i]->only_distinct : x[i]->only_total, all = pass ? x[i]->distinct : x[i]->total;
      const double q = mfx_histoQV((double)only, (double)all, rdb.k);
      snprintf(line, sizeof line, "%s\t%lu\t%lu\t%.4f\t%.6g\n", names[i], (unsigned long)only, (unsigned long)all, q, pow(10.0, q / -10.0));
      qv += line;
    }
  }
  if (!write_diploid_text(stem + ".qv", qv)) return 1;
  std::string cs = "# the solid read k-mers (-min <= count <= -max) an assembly holds: Merqury's k-mer completeness in spirit, unvalidated against Merqury\n#name\tall\tfound\tsolid\tpercent\n";
  for (int i = 0; i < 3; ++i) {
    snprintf(line, sizeof line, "%s\tall\t%lu\t%lu\t%.4f\n", names[i], (unsigned long)x[i]->found, (unsigned long)st.solid, st.solid ? 100.0 * (double)x[i]->found / (double)st.solid : 0.0);
    cs += line;
  }
  if (!write_diploid_text(stem + ".completeness.stats", cs)) return 1;
  if (peak)
    for (int i = 0; i < 3; ++i) {
      fprintf(stderr, "-- Compute completeness: %s.\n", names[i]);
      print_completeness(t64, u64 + 64 * i);
    }
  fprintf(stderr, "-- Joined: %lu read k-mers, %lu and %lu assembly k-mers, %lu in both assemblies, %lu window%s.\n", (unsigned long)st.n_read, (unsigned long)st.n_hap1,
          (unsigned long)st.n_hap2, (unsigned long)st.n_shared, (unsigned long)st.windows, st.windows == 1 ? "" : "s");
  fprintf(stderr, "Bye!\n");
  return 0;
}

// merfin -phase: hap-mer markers, phase blocks and switch errors (mfx_phase_run).  The table is the sequence-only index -- the k-mers of
// -sequence claimed, set A loaded update-only on the read side, set B on the assembly side; the assembly's own counts are not needed and
// are not counted -- or, for k > 31 and for a database that is not canonical, the full tables of the two sets.
static int run_phase(Globals &G) {
  mfx_db_info adb, bdb;
  if (mfx_db_probe(G.hapmers[0], &adb) || mfx_db_probe(G.hapmers[1], &bdb)) DIE_MFX("opening -hapmers");
  const int k = adb.k;
  fprintf(stderr, "-- Opening sequences in '%s'.\n", G.seqName);
  Sequences S;
  if (!S.start(G.seqName)) { fprintf(stderr, "ERROR: cannot open '%s'.\n", G.seqName); return 1; }
  if (!S.finish()) {
    fprintf(stderr, "ERROR: reading '%s' failed (read error, or the decompressor exited with an error: truncated or corrupt file?).\n", G.seqName);
    return 1;
  }
  Owned<mfx_seq, mfx_seq_free> seq;
  seq = mfx_seq_upload(G.device, S.bases.data(), S.lens.data(), S.size());
  if (!seq) DIE_MFX("uploading sequences");
  Owned<mfx_index, mfx_index_free> ix;
  int lrc = MFX_E_NONCANON;
  if (k <= 31) {
    const uint64_t capacity = S.totalBases + 1024;
    memory_banner(G, mfx_index_estimate_gb_for_seq(k, capacity));
    ix = mfx_index_create_for_seq_lf(k, capacity, G.maxMemory, G.device, 0.4);
    if (!ix) { fprintf(stderr, "\n%s\n\n", mfx_last_error()); return 1; }
    fprintf(stderr, "-- Claiming the %d-mers of '%s' on the GPU.\n", k, G.seqName);
    if (mfx_index_claim_seq(ix, seq, nullptr)) DIE_MFX("claiming sequence k-mers");
    for (int side = 0; side < 2; ++side) {
      fprintf(stderr, "-- Loading hap-mers %c from '%s' into lookup table.\n", "AB"[side], G.hapmers[side]);
      lrc = mfx_index_load_db(ix, G.hapmers[side], side, G.minV, G.maxV);
      if (lrc && lrc != MFX_E_NONCANON) DIE_MFX("loading -hapmers");
      if (lrc) break;
    }
    if (lrc) fprintf(stderr, "-- A k-mer database is not canonical; building the full lookup tables instead.\n");
  }
  if (lrc) {
    const uint64_t capacity = adb.n_kmers + bdb.n_kmers + 1024;
    memory_banner(G, mfx_index_estimate_gb(k, capacity));
    ix = mfx_index_create_lf(k, capacity, G.maxMemory, G.device, 0.7);
    if (!ix) { fprintf(stderr, "\n%s\n\n", mfx_last_error()); return 1; }
    for (int side = 0; side < 2; ++side) {
      fprintf(stderr, "-- Loading hap-mers %c from '%s' into lookup table.\n", "AB"[side], G.hapmers[side]);
      if (mfx_index_load_db(ix, G.hapmers[side], side, G.minV, G.maxV)) DIE_MFX("loading -hapmers");
    }
  }
  const mfx_kparams kp{1.0, 0, nullptr, nullptr};                 // (no K* is evaluated: mfx_phase_run does not read them)
  Owned<mfx_eval, mfx_eval_free> ev;
  ev = mfx_eval_create(ix, &kp, 0);
  if (!ev) DIE_MFX("creating evaluator");
  const mfx_phase_opts o{G.phSwitches, G.phRange};
  fprintf(stderr, "-- Phase blocks of the hap-mers (at most %lu switch markers within %lu bases stay inside a block) to '%s'.\n", (unsigned long)o.switches,
          (unsigned long)o.range, G.outName);
  Owned<mfx_phase, mfx_phase_free> res;
  {
    mfx_phase *r = nullptr;
    if (mfx_phase_run(ev, seq, &o, &r)) DIE_MFX("-phase");
    res = r;
  }
  std::vector<mfx_phase_block> recs((size_t)mfx_phase_count(res));
  std::vector<uint64_t> counts((size_t)S.size() * 4);
  if (mfx_phase_copy(res, recs.data(), recs.size()) || mfx_phase_contig_counts(res, counts.data(), S.size())) DIE_MFX("-phase");
  if (mfx_phase_write(recs.data(), recs.size(), counts.data(), seq, S.names.data(), k, &o, G.outName)) DIE_MFX("writing the phase blocks");
  uint64_t nb[2] = {0, 0}, nm[2] = {0, 0}, ns[2] = {0, 0}, span[2] = {0, 0};
  for (const mfx_phase_block &x : recs) { nb[x.hap]++; nm[x.hap] += x.n_hap + x.n_switch; ns[x.hap] += x.n_switch; span[x.hap] += x.end - 1 + (uint64_t)k - x.start; }
  for (int h = 0; h < 2; ++h)
    fprintf(stderr, "-- %c: %lu blocks, %lu bases, %lu markers, %lu switch markers.\n", "AB"[h], (unsigned long)nb[h], (unsigned long)span[h], (unsigned long)nm[h],
            (unsigned long)ns[h]);
  fprintf(stderr, "-- all: %lu blocks, %lu bases, %lu markers, %lu switch markers (switch rate %.6f).\n", (unsigned long)(nb[0] + nb[1]), (unsigned long)(span[0] + span[1]),
          (unsigned long)(nm[0] + nm[1]), (unsigned long)(ns[0] + ns[1]), nm[0] + nm[1] ? (double)(ns[0] + ns[1]) / (double)(nm[0] + nm[1]) : 0.0);
  fprintf(stderr, "Bye!\n");
  return 0;
}

// merfin -bin: per-read hap-mer counts and the reads sorted by parent (mfx_bin_*).  The table is the full table of the two sets, A on the
// read side and B on the assembly side, as in the second branch of run_phase.  The reads are parsed in chunks, added, taken and written:
// the host keeps only the records in flight -- under -split their bases, until their class is known.
static int run_bin(Globals &G) {
  mfx_db_info adb, bdb;
  if (mfx_db_probe(G.hapmers[0], &adb) || mfx_db_probe(G.hapmers[1], &bdb)) DIE_MFX("opening -hapmers");
  const int k = adb.k;
  const uint64_t capacity = adb.n_kmers + bdb.n_kmers + 1024;
  memory_banner(G, mfx_index_estimate_gb(k, capacity));
  Owned<mfx_index, mfx_index_free> ix;
  ix = mfx_index_create_lf(k, capacity, G.maxMemory, G.device, 0.7);
  if (!ix) { fprintf(stderr, "\n%s\n\n", mfx_last_error()); return 1; }
  // the norms of the class rule: the distinct k-mers each load puts into the table (a k-mer of B that A holds is a shared one: it is a hit
  // of neither set and adds to neither norm_b nor the classes)
  uint64_t norm[2] = {0, 0}, held = 0;
  for (int side = 0; side < 2; ++side) {
    fprintf(stderr, "-- Loading hap-mers %c from '%s' into lookup table.\n", "AB"[side], G.hapmers[side]);
    if (mfx_index_load_db(ix, G.hapmers[side], side, G.minV, G.maxV)) DIE_MFX("loading -hapmers");
    mfx_index_info info;
    if (mfx_index_get_info(ix, &info)) DIE_MFX("loading -hapmers");
    norm[side] = info.distinct - held;
    held = info.distinct;
  }
  const mfx_kparams kp{1.0, 0, nullptr, nullptr};                 // (no K* is evaluated: mfx_bin_* do not read them)
  Owned<mfx_eval, mfx_eval_free> ev;
  ev = mfx_eval_create(ix, &kp, 0);
  if (!ev) DIE_MFX("creating evaluator");
  const mfx_bin_opts o{norm[0], norm[1], G.binRatioMilli, G.binMinHits};
  std::string stem = G.outName, zsuf;                           // out.gz -> out.bin.tsv.gz
  if (mfx_suffix_tool(stem)) { const size_t dot = stem.rfind('.'); zsuf = stem.substr(dot); stem.resize(dot); }
  fprintf(stderr, "-- Hap-mer counts of every read (A: %lu k-mers, B: %lu; ratio %u.%03u, at least %u hits) to '%s.bin.tsv%s'.\n", (unsigned long)norm[0],
          (unsigned long)norm[1], G.binRatioMilli / 1000, G.binRatioMilli % 1000, G.binMinHits, stem.c_str(), zsuf.c_str());
  static const char *const splitNames[3] = {".hapA.fasta", ".hapB.fasta", ".unknown.fasta"};
  mfx_file tsv, split[3];
  std::vector<std::string> outNames;
  auto open_out = [&](mfx_file &fh, const std::string &name) {
    outNames.push_back(name);
    fh = mfx_open_writer(name.c_str(), false);
    if (!fh.f) fprintf(stderr, "ERROR: cannot open '%s' for writing.\n", name.c_str());
    return fh.f != nullptr;
  };
  bool ok = open_out(tsv, stem + ".bin.tsv" + zsuf);
  for (int c = 0; ok && G.binSplit && c < 3; ++c) ok = open_out(split[c], stem + splitNames[c] + zsuf);
  mfx_bin *bn = ok ? mfx_bin_begin(ev, (uint64_t)std::max(0, env_flag("MFX_BIN_BATCH"))) : nullptr;
  if (ok && !bn) { fprintf(stderr, "ERROR: -bin: %s\n", mfx_last_error()); ok = false; }
  if (ok) fprintf(tsv.f, "#read\tlength\tkmers\tA\tB\tshared\tclass\n");
  struct Pending { std::string name, bases; uint64_t len; };
  std::deque<Pending> pending;                                   // the records added and not yet taken, in input order
  uint64_t cls_reads[3] = {0, 0, 0}, cls_bases[3] = {0, 0, 0}, cls_hits[3][4] = {{0}};
  std::vector<mfx_bin_record> recs;
  std::vector<uint8_t> cls;
  double t_parse = 0, t_add = 0, t_write = 0;
  auto now = []() { return std::chrono::steady_clock::now(); };
  auto since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(now() - t).count(); };
  auto drain = [&]() {                                           // what is final is taken, classified and written
    const auto t0 = now();
    uint64_t n = mfx_bin_ready(bn);
    recs.resize((size_t)n);
    cls.resize((size_t)n);
    if (n && (mfx_bin_take(bn, recs.data(), n, &n) || mfx_bin_classify(recs.data(), n, &o, cls.data()))) {
      fprintf(stderr, "ERROR: -bin: %s\n", mfx_last_error());
      return false;
    }
    for (uint64_t i = 0; i < n; ++i) {
      const Pending &p = pending.front();
      const mfx_bin_record &r = recs[(size_t)i];
      const int c = cls[(size_t)i];
      fprintf(tsv.f, "%s\t%lu\t%u\t%u\t%u\t%u\t%c\n", p.name.c_str(), (unsigned long)p.len, r.kmers, r.a, r.b, r.shared, "ABU"[c]);
      if (G.binSplit) {
        fputc('>', split[c].f);
        fwrite(p.name.data(), 1, p.name.size(), split[c].f);
        fputc('\n', split[c].f);
        fwrite(p.bases.data(), 1, p.bases.size(), split[c].f);
        fputc('\n', split[c].f);
      }
      cls_reads[c]++;
      cls_bases[c] += p.len;
      cls_hits[c][0] += r.kmers; cls_hits[c][1] += r.a; cls_hits[c][2] += r.b; cls_hits[c][3] += r.shared;
      pending.pop_front();
    }
    t_write += since(t0);
    return true;
  };
  const uint64_t CHUNK_BASES = 32ull << 20, CHUNK_RECORDS = 1u << 16;
  std::vector<SeqRecord> chunk;
  std::vector<const char *> ptrs;
  std::vector<uint64_t> lens;
  auto submit = [&]() {
    const auto t0 = now();
    ptrs.resize(chunk.size());
    lens.resize(chunk.size());
    for (size_t i = 0; i < chunk.size(); ++i) { ptrs[i] = chunk[i].data(); lens[i] = chunk[i].size(); }
    const int rc = mfx_bin_add(bn, ptrs.data(), lens.data(), (uint64_t)chunk.size());
    t_add += since(t0);
    if (rc) { fprintf(stderr, "ERROR: -bin: %s\n", mfx_last_error()); return false; }
    for (SeqRecord &r : chunk) {
      Pending p;
      p.len = r.size();
      p.name = std::move(r.name);
      if (G.binSplit) p.bases.assign(r.data(), r.size());
      pending.push_back(std::move(p));
    }
    chunk.clear();
    return drain();
  };
  for (size_t f = 0; ok && f < G.readsNames.size(); ++f) {
    fprintf(stderr, "-- Reading '%s'.\n", G.readsNames[f]);
    SeqFile sf(G.readsNames[f]);
    if (!sf.ok()) { fprintf(stderr, "ERROR: cannot open '%s'.\n", G.readsNames[f]); ok = false; break; }
    uint64_t held_bases = 0;
    auto t0 = now();
    for (SeqRecord r; ok && sf.next(r); r = SeqRecord()) {
      held_bases += r.size();
      chunk.push_back(std::move(r));
      if (held_bases >= CHUNK_BASES || chunk.size() >= CHUNK_RECORDS) {
        t_parse += since(t0);
        ok = submit();
        held_bases = 0;
        t0 = now();
      }
    }
    t_parse += since(t0);
    if (ok && sf.finish() != 0) {
      fprintf(stderr, "ERROR: reading '%s' failed (read error, or the decompressor exited with an error: truncated or corrupt file?).\n", G.readsNames[f]);
      ok = false;
    }
    if (ok) ok = submit();
  }
  if (ok && mfx_bin_flush(bn)) { fprintf(stderr, "ERROR: -bin: %s\n", mfx_last_error()); ok = false; }
  if (ok) ok = drain();
  mfx_bin_stats st{};
  if (bn && mfx_bin_end(bn, &st) && ok) { fprintf(stderr, "ERROR: -bin: %s\n", mfx_last_error()); ok = false; }
  if (ok && !pending.empty()) { fprintf(stderr, "ERROR: -bin: internal error: %zu records were never final.\n", pending.size()); ok = false; }
  if (tsv.f && mfx_close(tsv) && ok) { fprintf(stderr, "ERROR: writing '%s' failed (stream error or the compressor exited with an error).\n", outNames[0].c_str()); ok = false; }
  for (int c = 0; c < 3; ++c)
    if (split[c].f && mfx_close(split[c]) && ok) {
      fprintf(stderr, "ERROR: writing '%s' failed (stream error or the compressor exited with an error).\n", outNames[1 + c].c_str());
      ok = false;
    }
  if (!ok) return 1;
  {
    const std::string name = stem + ".bin.stats" + zsuf;
    mfx_file fh = mfx_open_writer(name.c_str(), false);
    if (!fh.f) { fprintf(stderr, "ERROR: cannot open '%s' for writing.\n", name.c_str()); return 1; }
    fprintf(fh.f, "#ratio\t%u.%03u\tminhits\t%u\tk\t%d\tnorm_A\t%lu\tnorm_B\t%lu\n", G.binRatioMilli / 1000, G.binRatioMilli % 1000, G.binMinHits, k, (unsigned long)norm[0],
            (unsigned long)norm[1]);
    fprintf(fh.f, "#class\treads\tbases\tkmers\tA\tB\tshared\n");
    uint64_t all[6] = {0, 0, 0, 0, 0, 0};
    for (int c = 0; c < 3; ++c) {
      fprintf(fh.f, "%c\t%lu\t%lu\t%lu\t%lu\t%lu\t%lu\n", "ABU"[c], (unsigned long)cls_reads[c], (unsigned long)cls_bases[c], (unsigned long)cls_hits[c][0],
              (unsigned long)cls_hits[c][1], (unsigned long)cls_hits[c][2], (unsigned long)cls_hits[c][3]);
      all[0] += cls_reads[c]; all[1] += cls_bases[c];
      for (int j = 0; j < 4; ++j) all[2 + j] += cls_hits[c][j];
    }
    fprintf(fh.f, "all\t%lu\t%lu\t%lu\t%lu\t%lu\t%lu\n", (unsigned long)all[0], (unsigned long)all[1], (unsigned long)all[2], (unsigned long)all[3], (unsigned long)all[4],
            (unsigned long)all[5]);
    if (mfx_close(fh)) { fprintf(stderr, "ERROR: writing '%s' failed (stream error or the compressor exited with an error).\n", name.c_str()); return 1; }
  }
  for (int c = 0; c < 3; ++c)
    fprintf(stderr, "-- %s: %lu reads, %lu bases, %lu hits of A, %lu of B.\n", c == 0 ? "A" : c == 1 ? "B" : "unknown", (unsigned long)cls_reads[c], (unsigned long)cls_bases[c],
            (unsigned long)cls_hits[c][1], (unsigned long)cls_hits[c][2]);
  if (env_flag("MFX_CLI_TIMING") > 0)
    fprintf(stderr, "-- bin: %.3f s parsing, %.3f s batching / packing / waiting for a stage, %.3f s classifying and writing; device %.3f s kernel + %.3f s copy\n", t_parse,
            t_add, t_write, st.seconds_kernel, st.seconds_copy);
  fprintf(stderr, "Bye!\n");
  return 0;
}

static int report_hist(Run &R) {
  const Globals &G = R.G;
  fprintf(stderr, "-- Generate histogram of the k* metric to '%s'.\n", G.outName);
  mfx_hist_result r;
  if (G.devices.size() > 1) {
    // one process, N devices (the reference drives all its workers from one binary, merfin.C:366-414): replicas of
    // the table and of the packed assembly by peer copy, every device evaluates its block-cyclic share
    const size_t N = G.devices.size();
    Slots S;
    int bad = S.make(G, R.ix, R.seq, R.ev, &R.kp) ? 0 : 1;
    R.clock.lap("replicate index");
    fprintf(stderr, "-- Evaluating on %zu devices.\n", N);
    if (!bad && mfx_hist_run_multi(S.evs.data(), S.sqs.data(), (uint32_t)N, &r)) bad = 1;
    std::string why = bad ? mfx_last_error() : "";
    S.release();
    if (bad) { fprintf(stderr, "ERROR: -hist on %zu devices: %s\n", N, why.c_str()); return 1; }
  } else if (R.streamHist) {
    if (mfx_hist_run_streamed(R.ev, R.seq, R.S.bases.data(), &r)) DIE_MFX("-hist");
  } else if (mfx_hist_run(R.ev, R.seq, &r)) DIE_MFX("-hist");
  if (!print_hist(R.S.recs, r, R.k, G.outName)) DIE_MFX("writing histogram");
  mfx_hist_result_free(&r);
  return 0;
}

static int report_dump(Run &R) {
  const Globals &G = R.G;
  const std::vector<SeqRecord> &recs = R.S.recs;
  fprintf(stderr, "-- Dump per-base k* metric to '%s'.\n", G.outName);
  ContigCounts counts;
  if (G.skipMissing) {
    // merfin-dump.C:34,81-87: -skipMissing suppresses the dump file entirely; only the counts remain
    mfx_hist_result r;
    if (mfx_hist_run(R.ev, R.seq, &r)) DIE_MFX("-dump -skipMissing");
    counts.lines(recs, r);
    mfx_hist_result_free(&r);
  } else if (G.devices.size() > 1) {
    // per-contig ordered output on N devices: a contiguous run of contigs per slot (balanced by bases), one host
    // thread per slot writes its part, the parts are concatenated in slot order
    const size_t N = G.devices.size();
    Slots S;
    if (!S.make(G, R.ix, R.seq, R.ev, &R.kp)) { fprintf(stderr, "ERROR: -dump on %zu devices: %s\n", N, mfx_last_error()); return 1; }
    R.clock.lap("replicate index");
    fprintf(stderr, "-- Evaluating on %zu devices.\n", N);
    const auto runs = contig_partition(std::vector<double>(R.S.lens.begin(), R.S.lens.end()), N);
    std::vector<std::string> parts(N), errs(N);
    std::vector<uint64_t> ka(recs.size(), 0), km(recs.size(), 0);
    std::vector<std::thread> th;
    for (size_t d = 0; d < N; ++d) {
      char suf[32];
      snprintf(suf, sizeof(suf), ".part%04zu", d);
      parts[d] = std::string(G.outName) + suf;
      th.emplace_back([&, d]() {
        mfx_host_threads_share((unsigned)N);
        for (size_t c = runs[d].first; c < runs[d].second; ++c)
          if (mfx_dump_contig(S.evs[d], S.sqs[d], (uint32_t)c, R.S.names[c], parts[d].c_str(), c > runs[d].first, &ka[c], &km[c])) { errs[d] = mfx_last_error(); return; }
      });
    }
    for (auto &x : th) x.join();
    S.release();
    for (size_t d = 0; d < N; ++d) if (!errs[d].empty()) { fprintf(stderr, "ERROR: -dump (slot %zu): %s\n", d, errs[d].c_str()); return 1; }
    if (!concat_parts(G.outName, parts, false)) { fprintf(stderr, "ERROR: cannot write '%s'.\n", G.outName); return 1; }
    for (size_t c = 0; c < recs.size(); ++c) counts.line(R.S.names[c], ka[c], km[c]);     // (the runs are the contigs in order)
  } else {
    for (size_t c = 0; c < recs.size(); ++c) {
      uint64_t ka = 0, km = 0;
      if (mfx_dump_contig(R.ev, R.seq, (uint32_t)c, R.S.names[c], G.outName, c > 0, &ka, &km)) DIE_MFX("-dump");
      counts.line(R.S.names[c], ka, km);
    }
    if (recs.empty()) { FILE *f = fopen(G.outName, "w"); if (f) fclose(f); }
  }
  return 0;
}

// K* per window of every contig, reduced on the device (mfx_track_run): what the README's "Assess collapses and duplications"
// makes from the -dump text with awk and wigToBigWig.  The counts on stderr are those of -dump -skipMissing.
static int report_track(Run &R) {
  const Globals &G = R.G;
  const size_t NC = R.S.recs.size();
  // (a compressed -output name -- out.gz / .bz2 / .xz -- keeps its suffix at the end of the three names: out.track.tsv.gz)
  std::string stem = G.outName, zsuf;
  if (mfx_suffix_tool(stem)) { const size_t dot = stem.rfind('.'); zsuf = stem.substr(dot); stem.resize(dot); }
  const std::string tsvName = stem + ".track.tsv" + zsuf, bgName = stem + ".kstar.bedgraph" + zsuf, missName = stem + ".missing.bedgraph" + zsuf;
  fprintf(stderr, "-- Summarise the k* metric per window of %lu positions to '%s', '%s' and '%s'.\n", (unsigned long)G.window, tsvName.c_str(),
          bgName.c_str(), missName.c_str());
  const uint64_t nw = mfx_track_num_windows(R.seq, G.window);
  std::vector<mfx_track_window> win((size_t)nw);
  uint64_t got = 0, kasm = 0, kmissing = 0;
  if (mfx_track_run(R.ev, R.seq, G.window, win.data(), nw, &got, &kasm, &kmissing)) DIE_MFX("-track");
  if (mfx_track_write(win.data(), got, R.seq, R.S.names.data(), G.window, tsvName.c_str(), bgName.c_str())) DIE_MFX("writing the windows");
  mfx_file mf = mfx_open_writer(missName.c_str(), false);
  if (!mf.f) { fprintf(stderr, "ERROR: cannot open '%s' for writing.\n", missName.c_str()); return 1; }
  fprintf(mf.f, "track type=bedGraph name=\"missing\"\n");
  std::vector<uint64_t> cmiss(NC, 0), casm(NC, 0);
  size_t i = 0;
  for (size_t c = 0; c < NC; ++c)
    for (uint64_t start = 0; start < R.S.lens[c]; start += G.window, ++i) {
      const mfx_track_window &w = win[i];
      cmiss[c] += w.n_missing;
      casm[c] += w.n_kmers;
      if (w.n_kmers)
        fprintf(mf.f, "%s\t%lu\t%lu\t%.6f\n", R.S.names[c], (unsigned long)start, (unsigned long)std::min<uint64_t>(start + G.window, R.S.lens[c]),
                (double)w.n_missing / (double)w.n_kmers);
    }
  if (mfx_close(mf)) { fprintf(stderr, "ERROR: writing '%s' failed.\n", missName.c_str()); return 1; }
  ContigCounts counts;
  for (size_t c = 0; c < NC; ++c) counts.line(R.S.names[c], casm[c], cmiss[c]);
  if (counts.cumAsm != kasm || counts.cumMissing != kmissing) {
    fprintf(stderr, "ERROR: -track: the windows hold %lu k-mers (%lu missing), the device counted %lu (%lu).\n", (unsigned long)counts.cumAsm,
            (unsigned long)counts.cumMissing, (unsigned long)kasm, (unsigned long)kmissing);
    return 1;
  }
  return 0;
}

// Runs of missing, collapsed and expanded k-mers as intervals, made on the device (mfx_regions_run): what the README's "Assess collapses and
// duplications" makes from the -dump text with awk.  The counts on stderr are those of -dump -skipMissing.
static int report_regions(Run &R) {
  const Globals &G = R.G;
  std::string stem = G.outName, zsuf;
  if (mfx_suffix_tool(stem)) { const size_t dot = stem.rfind('.'); zsuf = stem.substr(dot); stem.resize(dot); }
  const std::string bedName = stem + ".regions.bed" + zsuf;
  fprintf(stderr, "-- Runs of missing k-mers and of k-mers with |k*| >= %g (gap %lu, at least %lu k-mers) to '%s'.\n", G.regKstar, (unsigned long)G.regGap,
          (unsigned long)G.regMinrun, bedName.c_str());
  const mfx_regions_opts o{G.regKstar, G.regGap, G.regMinrun};
  Owned<mfx_regions, mfx_regions_free> res;
  uint64_t kasm = 0, kmissing = 0;
  {
    mfx_regions *r = nullptr;
    if (mfx_regions_run(R.ev, R.seq, &o, &r, &kasm, &kmissing)) DIE_MFX("-regions");
    res = r;
  }
  std::vector<mfx_region> recs((size_t)mfx_regions_count(res));
  if (mfx_regions_copy(res, recs.data(), recs.size())) DIE_MFX("-regions");
  if (mfx_regions_write(recs.data(), recs.size(), R.seq, R.S.names.data(), R.k, bedName.c_str())) DIE_MFX("writing the regions");
  // the per-contig counts: those of a -hist run, as -dump -skipMissing takes them
  mfx_hist_result h;
  if (mfx_hist_run(R.ev, R.seq, &h)) DIE_MFX("-regions (counts)");
  ContigCounts counts;
  counts.lines(R.S.recs, h);
  mfx_hist_result_free(&h);
  if (counts.cumAsm != kasm || counts.cumMissing != kmissing) {
    fprintf(stderr, "ERROR: -regions: the contigs hold %lu k-mers (%lu missing), the class pass counted %lu (%lu).\n", (unsigned long)counts.cumAsm,
            (unsigned long)counts.cumMissing, (unsigned long)kasm, (unsigned long)kmissing);
    return 1;
  }
  static const char *const cls_name[3] = {"missing", "collapsed", "expanded"};
  uint64_t nr[3] = {0, 0, 0}, nk[3] = {0, 0, 0}, nb[3] = {0, 0, 0};
  for (const mfx_region &x : recs) { nr[x.cls]++; nk[x.cls] += x.n_kmers; nb[x.cls] += x.end - 1 + (uint64_t)R.k - x.start; }
  for (int c = 0; c < 3; ++c)
    fprintf(stderr, "-- %s: %lu regions, %lu flagged k-mers, %lu bases covered.\n", cls_name[c], (unsigned long)nr[c], (unsigned long)nk[c], (unsigned long)nb[c]);
  return 0;
}

// The call set of the variant modes in several slots: one pass over the VCF gives the records per contig (for the balance), and the lines
// themselves, so that every slot is handed a VCF of ITS contigs only (each slot parsing all 4 M records of a human call set made N slots
// N times the host work of one; the host is what bounds these modes)
struct VcfBySlot {
  std::string vtext;
  std::vector<std::pair<size_t, size_t>> vhead;                          // header lines (offset, length incl. newline)
  std::vector<std::vector<std::pair<size_t, size_t>>> vlines;           // data lines per contig, in file order
  std::vector<double> w;                                                // the weight of every contig: its records

  int read(const char *vcfName, const Sequences &S) {
    const std::vector<SeqRecord> &recs = S.recs;
    w.assign(recs.size(), 0.0);
    vlines.resize(recs.size());
    mfx_file vf = mfx_open_reader(vcfName);
    if (!vf.f) { fprintf(stderr, "ERROR: cannot open VCF '%s'.\n", vcfName); return 1; }
    {
      std::vector<char> blk(1 << 22);
      size_t n;
      while ((n = fread(blk.data(), 1, blk.size(), vf.f)) > 0) vtext.append(blk.data(), n);
    }
    if (mfx_close(vf)) { fprintf(stderr, "ERROR: reading VCF '%s' failed.\n", vcfName); return 1; }
    std::vector<std::pair<std::string, size_t>> idx;
    for (size_t c = 0; c < recs.size(); ++c) idx.emplace_back(recs[c].name, c);
    std::sort(idx.begin(), idx.end());
    size_t last_c = recs.size();
    std::string last_chr;
    for (size_t o = 0; o < vtext.size();) {
      const char *nl = (const char *)memchr(vtext.data() + o, '\n', vtext.size() - o);
      const size_t e = nl ? (size_t)(nl - vtext.data()) + 1 : vtext.size(), n = e - o;
      if (vtext[o] == '#') vhead.emplace_back(o, n);
      else if (n > 1) {
        const char *tab = (const char *)memchr(vtext.data() + o, '\t', n);
        if (tab) {
          const size_t cl = (size_t)(tab - (vtext.data() + o));
          if (last_c == recs.size() || last_chr.size() != cl || memcmp(last_chr.data(), vtext.data() + o, cl) != 0) {
            last_chr.assign(vtext.data() + o, cl);
            auto it = std::lower_bound(idx.begin(), idx.end(), std::make_pair(last_chr, (size_t)0));
            last_c = (it != idx.end() && it->first == last_chr) ? it->second : recs.size() + 1;   // + 1: not a contig of -sequence
          }
          if (last_c < recs.size()) { w[last_c] += 1.0; vlines[last_c].emplace_back(o, n); }
        }
      }
      o = e;
    }
    for (size_t c = 0; c < recs.size(); ++c) w[c] += 1e-9 * (double)S.lens[c];
    return 0;
  }
  // a slot's VCF: all header lines + the lines of its contigs [run.first, run.second)
  bool write(const std::string &path, std::pair<size_t, size_t> run) const {
    FILE *vf = fopen(path.c_str(), "w");
    bool ok = vf != nullptr;
    for (const auto &h : vhead) ok = ok && fwrite(vtext.data() + h.first, 1, h.second, vf) == h.second;
    for (size_t c = run.first; c < run.second && ok; ++c)
      for (const auto &l : vlines[c]) {
        ok = ok && fwrite(vtext.data() + l.first, 1, l.second, vf) == l.second;
        if (ok && vtext[l.first + l.second - 1] != '\n') ok = fputc('\n', vf) != EOF;     // a last line without newline
      }
    if (vf && fclose(vf) != 0) ok = false;
    return ok;
  }
};

// open_Inputs + processVariants + outputVariants (merfin-globals.C:201-219, merfin-variants.C:131-345)
static int report_variants(Run &R) {
  Globals &G = R.G;
  const Sequences &Q = R.S;
  fprintf(stderr, "-- Opening vcf file '%s'.\n", G.vcfName);
  fprintf(stderr, "-- Generate variant mers and score them.\n");
  const std::string outName = std::string(G.outName) + (G.reportType == OP_POLISH ? ".polish.vcf" : ".filter.vcf");   // :324-327
  const std::string dbgName = std::string(G.outName) + ".00.debug.gz";
  const mfx_variant_opts vo = variant_opts(G, G.debug ? dbgName.c_str() : nullptr);
  uint64_t ncl = 0;
  // One device is run as ONE slot.  (Rounds 2-3 ran it as 4 slots sharing its table: the host phases of these modes then
  // alternated between parallel and serial stretches and several slots filled one another's gaps -- 1 Gb: 2.0 s in 8 slots
  // against 2.7 s in one.  With the host side of round 4 -- arenas per run of clusters, parallel VCF load, device scoring --
  // one slot on all host threads is at least as fast and needs neither the per-slot VCF files nor the evaluator replicas:
  // config 4 at 3 Gb, evaluate + write 1.11-1.14 s in one slot, 1.16-1.19 s in four + 0.13-0.15 s to set the slots up,
  // profiles/r04_cfg4_fullsize.txt.)  MFX_VARIANT_SLOTS overrides; several -devices are one slot each.
  {
    const size_t want = variant_slots(G);
    const std::vector<int> real = G.devices;
    while (G.devices.size() < want) G.devices.push_back(real[G.devices.size() % real.size()]);
  }
  if (G.devices.size() > 1) {
    // BASELINE config 4 names 8 GPUs: contigs cut into one contiguous run per slot, balanced by their VCF records;
    // every slot scores its clusters on its own device and writes its part; one VCF header in the concatenation
    const size_t N = G.devices.size();
    VcfBySlot V;
    if (V.read(G.vcfName, Q)) return 1;
    Slots S;
    if (!S.make(G, R.ix, nullptr, R.ev, &R.kp)) { fprintf(stderr, "ERROR: variant scoring on %zu devices: %s\n", N, mfx_last_error()); return 1; }
    R.clock.lap("replicate index");
    fprintf(stderr, "-- Evaluating in %zu slots.\n", N);
    const auto runs = contig_partition(V.w, N);
    std::vector<std::string> parts(N), errs(N), dbgs(N), vins(N), logs(N);
    std::vector<uint64_t> ncls(N, 0);
    auto drop_parts = [&]() { for (size_t e = 0; e < N; ++e) { if (!parts[e].empty()) remove(parts[e].c_str()); if (!vins[e].empty()) remove(vins[e].c_str()); if (!logs[e].empty()) remove(logs[e].c_str()); } };
    std::vector<std::thread> th;
    for (size_t d = 0; d < N; ++d) {
      char suf[48];
      snprintf(suf, sizeof(suf), ".part%04zu.in.vcf", d);
      vins[d] = outName + suf;
      if (!V.write(vins[d], runs[d])) { fprintf(stderr, "ERROR: cannot write '%s'.\n", vins[d].c_str()); drop_parts(); return 1; }
    }
    std::string().swap(V.vtext);
    for (size_t d = 0; d < N; ++d) {
      char suf[48];
      snprintf(suf, sizeof(suf), ".part%04zu", d);
      parts[d] = outName + suf;
      snprintf(suf, sizeof(suf), ".%02zu.debug.gz", d);
      dbgs[d] = std::string(G.outName) + suf;
      // every slot logs to its own file; they are replayed on stderr in slot order once all slots are done (N slots
      // writing PANIC / progress lines to one stderr interleave them mid-line)
      logs[d] = parts[d] + ".log";
      th.emplace_back([&, d]() {
        mfx_host_threads_share((unsigned)N);                 // N slots side by side: each takes its share of the host threads
        mfx_variant_opts o = vo;
        o.debug_path = G.debug ? dbgs[d].c_str() : nullptr;
        const size_t lo = runs[d].first, hi = runs[d].second;
        if (mfx_variants_run(S.evs[d], vins[d].c_str(), Q.names.data() + lo, Q.bases.data() + lo, Q.lens.data() + lo, (uint32_t)(hi - lo), &o, parts[d].c_str(),
                             logs[d].c_str(), &ncls[d]))
          errs[d] = mfx_last_error();
      });
    }
    for (auto &x : th) x.join();
    for (size_t d = 0; d < N; ++d) {
      remove(vins[d].c_str());
      vins[d].clear();
      if (FILE *lf = fopen(logs[d].c_str(), "r")) {
        if (N > 1) fprintf(stderr, "-- slot %zu (contigs %zu..%zu):\n", d, runs[d].first, runs[d].second);
        char lb[1 << 14];
        size_t n;
        while ((n = fread(lb, 1, sizeof(lb), lf)) > 0) fwrite(lb, 1, n, stderr);
        fclose(lf);
      }
      remove(logs[d].c_str());
      logs[d].clear();
    }
    S.release();
    for (size_t d = 0; d < N; ++d) if (!errs[d].empty()) { fprintf(stderr, "ERROR: variant scoring (slot %zu): %s\n", d, errs[d].c_str()); drop_parts(); return 1; }
    if (!concat_parts(outName, parts, true)) { fprintf(stderr, "ERROR: cannot write '%s'.\n", outName.c_str()); drop_parts(); return 1; }
    for (uint64_t x : ncls) ncl += x;
  } else if (R.vcfReady || R.vcfAhead.f.valid()) {
    Owned<mfx_vcf, mfx_vcf_free> vcf;
    vcf = R.vcfReady ? R.vcfReady.release() : R.vcfAhead.f.get();
    if (!vcf) { fprintf(stderr, "ERROR: variant scoring: %s\n", R.vcfAheadError.c_str()); return 1; }
    const int vrc = mfx_variants_run_vcf(R.ev, vcf, Q.names.data(), Q.bases.data(), Q.lens.data(), Q.size(), &vo, outName.c_str(), nullptr, &ncl);
    // (leaving the 4 M records to the process's exit instead of freeing them here was measured: 0.1 s less in this phase, the same wall --
    // profiles/r05_exit_ab.txt)
    vcf.reset();
    if (vrc) DIE_MFX("variant scoring");
  } else if (mfx_variants_run(R.ev, G.vcfName, Q.names.data(), Q.bases.data(), Q.lens.data(), Q.size(), &vo, outName.c_str(), nullptr, &ncl))
    DIE_MFX("variant scoring");
  return 0;
}

static int report_completeness(Run &R) {
  fprintf(stderr, "-- Compute completeness.\n");
  double t64[64], u64[64];
  if (mfx_completeness_pieces(R.ev, t64, u64)) DIE_MFX("-completeness");
  print_completeness(t64, u64);
  return 0;
}

int main(int argc, char **argv) {
  const double stamp_main = epoch();
  Globals G;
  Errors err;
  // 1. parse, check (every refusal before a device is touched), dispatch the operations that are not reports
  parse_args(argc, argv, G, err);
  check_diploid_flags(G, err);
  if (diploid_named(G)) {
    if (!err.empty()) return fail_usage(argv[0], err, false, false, false, false, false, false, false, true);
    if (G.peakGiven && !load_Kmetric(G)) return 1;             // (host only, before the HIP runtime starts: see below)
    return devices_available({G.device}) ? run_diploid(G) : 1;
  }
  check_trio_flags(G, err);
  if (trio_named(G)) {
    if (!err.empty()) return fail_usage(argv[0], err, false, false, false, false, false, false, true);
    if (!G.devices.empty()) G.device = G.devices[0];
    if (!devices_available({G.device})) return 1;
    return G.trio ? run_trio(G) : run_histogram(G);
  }
  check_bin_flags(G, err);
  if (bin_named(G)) {
    if (!err.empty()) return fail_usage(argv[0], err, false, false, false, false, false, true);
    if (!G.devices.empty()) G.device = G.devices[0];
    return devices_available({G.device}) ? run_bin(G) : 1;
  }
  check_phase_flags(G, err);
  if (phase_named(G)) {
    if (!err.empty()) return fail_usage(argv[0], err, false, false, false, true);
    if (!G.devices.empty()) G.device = G.devices[0];
    return devices_available({G.device}) ? run_phase(G) : 1;
  }
  check_merge_flags(G, err);
  if (!G.mergeNames.empty() || G.opName || !G.notNames.empty())
    return err.empty() ? run_merge(G) : fail_usage(argv[0], err, true, false, false, false, !G.notNames.empty());
  check_count_flags(G, err);
  if (G.count) return err.empty() ? run_count(G) : fail_usage(argv[0], err);
  check_join_flags(G, err);
  if (G.join && !G.readsNames.empty()) return fail_usage(argv[0], err, false, true);      // (the checks of -reads open -seqmers for its k)
  if (!check_reads_flags(G, err)) return 1;
  check_track_flags(G, err);
  check_regions_flags(G, err);
  check_spectrum_flags(G, err);
  check_peak_auto_flags(G, err);
  if (G.convertName && err.empty()) return run_convert(G);
  check_report_flags(G, err);
  if (!err.empty()) return fail_usage(argv[0], err, false, G.join, regions_named(G));
  if (!G.devices.empty()) G.device = G.devices[0];
  else G.devices.push_back(G.device);
  // 2. load_Kmetric first (merfin-globals.C:21-62 runs before the databases are opened; host only -- a compressed table's decompressor has
  // come and gone before the HIP runtime starts)
  if (!load_Kmetric(G)) return 1;
  // 3. (the device check stays on this thread, before anything else is started: see devices_available)
  if (!devices_available(G.devices)) return 1;
  if (G.join) return run_join(G);
  Run R(G);
  R.clock.start(stamp_main);
  // 4. the databases are probed: the read DB defines k
  if (probe_databases(R)) return 1;
  // 5. the stage of the read database begins
  // (MFX_CLI_STAGE_FIRST=0: the stage begins after the device is warmed up.  Measured, profiles/r05_stager_diag.txt: the warm-up then takes
  // 0.06 instead of 0.25 s, but the 0.15-0.2 s that the process's first allocations / queue / kernel cost move into the stager's start, the
  // claim kernel is launched at the same 0.35 s, and with stager, FASTA reader and encoder all at full speed in the first 0.3 s the process
  // runs into the CPU quota of a 16-core box in some runs: 1.09-1.13 s or 1.27-1.29 s against 1.12-1.16 s this way)
  const bool stageFirst = env_flag("MFX_CLI_STAGE_FIRST") != 0;
  if (stageFirst) begin_stage(R);
  R.clock.lap("probe k-mer databases");
  // 6. the FASTA reader starts: its own thread from here on
  if (G.seqName) {
    fprintf(stderr, "-- Opening sequences in '%s'.\n", G.seqName);
    if (!R.S.start(G.seqName)) { fprintf(stderr, "ERROR: cannot open '%s'.\n", G.seqName); return 1; }
  }
  // 7. which index: path-only (its VCF then loads beside the FASTA reader), sequence-only or full; the sequence first or under the build
  if (decide_path_only(R)) return 1;
  const bool compressed = G.seqName && mfx_suffix_tool(G.seqName) != nullptr;
  decide_seq_only_and_defer(R, compressed);
  // 8. while the reader thread is on the file: the device's context, the library's code object and the pinned-memory path come
  // up here instead of inside the first upload (~0.07 s; an error here is left to that upload to report).  Not with a
  // decompressor child around (see the device check above) and not for several devices (their slots come up in parallel).
  if (G.seqName && !compressed && G.devices.size() == 1 && env_flag("MFX_CLI_WARM") != 0) (void)mfx_device_warm(G.device);
  if (!stageFirst) begin_stage(R);
  // 9. the sequence is waited for, or left to read under the index build
  if (!R.deferSeq && finish_seq(R)) return 1;
  if (R.pathOnly) begin_path_stages(R);
  // 10. -sharded is a run of its own
  if (G.sharded) return run_on_shards(R);
  // 11. upload.  The variant modes never evaluate the assembly itself on the device -- the paths around the variants go up batch by batch
  // (mfx_variants_run takes the host bases) --, so the assembly is uploaded only if its k-mers must be counted there (no
  // -seqmers: the counting branch of the build makes the upload when it gets there).  3 Gb: 0.2 s and 1.1 GB of HBM not spent.
  R.streamHist = G.reportType == OP_HIST && G.seqDBname && G.devices.size() == 1 && !R.seqOnly;
  const bool seqOnDevice = !R.variantMode;
  if (!R.deferSeq && seqOnDevice && !make_seq(R)) DIE_MFX("uploading sequences");
  // 12. the VCF of the variant modes loads ahead, under the index build
  start_vcf_ahead(R);
  // 13. the image of the index, or its build.  The path-only index falls back to the full tables when the device could not take it or a
  // database is not canonical (the prepared call set runs on the full tables as well); the sequence-only index when a database is not
  // canonical: what -index saves is then the full index of these inputs
  if (load_index_image(R)) return 1;
  if (!R.ix && (R.pathOnly || R.seqOnly)) {
    const int brc = R.pathOnly ? build_path_only_index(R) : build_seq_only_index(R);
    if (brc > 0) return brc;
    if (brc < 0) { R.pathOnly = R.seqOnly = false; R.fingerprint = R.fingerprintFull; }
  }
  if (!R.ix && build_full_index(R)) return 1;
  R.clock.lap("build / load index");
  if (R.deferSeq && !R.seq) {
    if (finish_seq(R)) return 1;
    if (seqOnDevice && !make_seq(R)) DIE_MFX("uploading sequences");
  }
  // 14. -spectrum / -peak auto
  if ((G.reportType == OP_SPECTRUM || G.peakAuto) && run_spectrum_or_peak(R)) return 1;
  // 15. the evaluator
  R.kp = mfx_kparams{G.peak, (uint32_t)G.copyKmerK.size(), G.copyKmerK.data(), G.copyKmerP.data()};
  if (G.reportType != OP_SPECTRUM) {
    R.ev = mfx_eval_create(R.ix, &R.kp, 0);
    if (!R.ev) DIE_MFX("creating evaluator");
  }
  // 16. the report
  const int rc = G.reportType == OP_HIST ? report_hist(R) : G.reportType == OP_DUMP ? report_dump(R) : G.reportType == OP_TRACK ? report_track(R) :
                 G.reportType == OP_REGIONS ? report_regions(R) :
                 R.variantMode ? report_variants(R) : G.reportType == OP_COMPL ? report_completeness(R) : 0;
  if (rc) return rc;
  R.clock.lap("evaluate + write");
  // 17. release
  R.ev.reset();
  R.seq.reset();
  R.ix.reset();
  R.clock.lap("release");
  // 18. timing, 19. Bye!
  R.clock.print();
  fprintf(stderr, "Bye!\n");
  // MFX_CLI_QUICK_EXIT=1: every output is written and closed by now; leave without the tear-down of the HIP runtime's statics
  // (not under a profiler: its tool library writes its files from an exit handler)
  if (env_flag("MFX_CLI_QUICK_EXIT") > 0) { fflush(nullptr); _exit(0); }
  return 0;
}
