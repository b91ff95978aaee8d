// merfin (MI355X) -- the command line: the flags (Globals), their parser and the checks that refuse a run before any device is touched.
#pragma once
#include <ctype.h>
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "../../include/merfin_amd.h"

enum { OP_NONE, OP_HIST, OP_COMPL, OP_DUMP, OP_FILTER, OP_POLISH, OP_BETTER, OP_STRICT, OP_LOOSE, OP_TRACK, OP_SPECTRUM, OP_REGIONS };

struct Globals {
  const char *seqName = nullptr, *seqDBname = nullptr, *readDBname = nullptr, *pLookupTable = nullptr;
  const char *vcfName = nullptr, *outName = nullptr, *indexName = nullptr, *convertName = nullptr;
  bool placed = false;                 // -convert -placed: the records sorted by their place in the -hist table (mfx_db_convert_placed)
  double peak = 0, maxMemory = 0;
  uint64_t minV = 0, maxV = ~0ull;
  int threads = 0, reportType = OP_NONE, device = 0;
  std::vector<int> devices;          // -devices: the GPUs of this node one process drives (-hist); [0] == device
  unsigned comb = 15;
  bool nosplit = false, debug = false, skipMissing = false, sharded = false;
  std::vector<uint32_t> copyKmerK;
  std::vector<double> copyKmerP;
  std::vector<const char *> readsNames;  // -reads: the read counts from these FASTA / FASTQ files instead of -readmers
  int kArg = 0;                          // -k (0: not given); with -reads: the run's k once the flags are checked
  uint64_t window = 1000;                // -window: k-mer start positions per window of -track
  bool windowGiven = false;
  bool peakAuto = false;                 // -peak auto: the haploid peak is read off the index's copy-number spectrum (mfx_spectrum_peak)
  uint32_t copies = 4, maxMult = 10000;  // -copies / -maxmult of -spectrum
  bool copiesGiven = false, maxMultGiven = false;
  bool count = false;                    // -count: no report; the k-mers of -reads counted on the GPU and written as a database
  bool peakGiven = false, devicesGiven = false;
  bool passesGiven = false, passesAuto = false;   // -count -passes P|auto: the k-mers counted in passes over key ranges
  uint32_t passes = 1;
  std::vector<const char *> mergeNames;  // -merge: no report; these sorted databases combined on the GPU into -output (mfx_db_merge)
  std::vector<const char *> notNames;    // -not of -merge: databases whose k-mers are not written (mfx_db_merge_except)
  const char *opName = nullptr;          // -op of -merge: sum (default), max, min, intersect
  int mergeOp = MFX_MERGE_SUM;
  double regKstar = 1.0;                 // -kstar: |K*| at which -regions calls a k-mer collapsed / expanded
  uint64_t regGap = 0, regMinrun = 1;    // -gap / -minrun of -regions
  bool kstarGiven = false, gapGiven = false, minrunGiven = false;
  bool phase = false;                    // -phase: no K* report; hap-mer markers, phase blocks and switch errors of -sequence (mfx_phase_run)
  std::vector<const char *> hapmers;     // -hapmers: the two sets of haplotype-specific k-mers (A, then B)
  uint64_t phSwitches = 100, phRange = 20000;   // -switches / -range of -phase
  bool switchesGiven = false, rangeGiven = false;
  bool bin = false;                      // -bin: no K* report; per-read hap-mer counts of -reads, the reads sorted by parent (mfx_bin_*)
  uint32_t binRatioMilli = 1000, binMinHits = 1;   // -ratio (in thousandths) / -minhits of -bin
  bool ratioGiven = false, minhitsGiven = false, binSplit = false;      // -split: the reads themselves written per class
  bool join = false;                     // -join: -completeness / -spectrum as the sorted join of two sorted databases, no table (mfx_db_join_*)
  bool diploid = false;                  // -diploid: two haplotype assemblies (-hap1 / -hap2) against -readmers in one join (mfx_db_diploid)
  std::vector<const char *> hap1Names, hap2Names;      // every -hap1 / -hap2 given (exactly one each is taken)
  int readmersGiven = 0;                 // how often -readmers was named
  bool trio = false;                     // -trio: no report; the two hap-mer databases of -mat / -pat [/ -child] in one pass (mfx_db_trio)
  const char *matName = nullptr, *patName = nullptr, *childName = nullptr;
  uint32_t cutMat = 0, cutPat = 0, cutChild = 0;      // -cutmat / -cutpat / -cutchild of -trio; 0: auto (the valley of the k-mer histogram)
  bool cutMatGiven = false, cutPatGiven = false, cutChildGiven = false;
  const char *histName = nullptr;        // -histogram db: no report; the k-mer histogram of a sorted database (mfx_db_histogram)
};

typedef std::vector<std::string> Errors;

static void usage(const char *exe) {
  fprintf(stderr,
          "usage: %s <report-type> -sequence <seq.fasta> -readmers <read.meryl> -peak <haploid_peak>\n"
          "          [-prob <lookup_table>] [-seqmers <seq.meryl>] [-vcf <input.vcf>] -output <output>\n\n"
          "  Evaluates every k-mer of <seq.fasta> against the read k-mer database on an MI355X GPU.\n"
          "  Inputs: FASTA/FASTQ, plain or gz/bz2/xz.  K-mer databases: meryl directory, `meryl print`\n"
          "  text, or the flat binary written by mfx_db_write_flat.  k is taken from -readmers.\n\n"
          "    -min m / -max m   ignore read k-mers with value below / above m\n"
          "    -memory m         do not use more than m GB (of HBM) for the k-mer tables\n"
          "    -threads t        accepted for compatibility (host threads)\n"
          "    -peak m           haploid k-mer coverage peak (required except -filter and -spectrum)\n"
          "    -peak auto        -hist, -dump, -track, -spectrum on one device: the peak is read off the single-copy row of the index's\n"
          "                      copy-number spectrum (one more pass over the table on the GPU) and reported on stderr\n"
          "    -prob file        readK,prob rows; row n overrides -peak for multiplicity n\n"
          "    -seqmers db       assembly k-mer database; default: counted from -sequence on the GPU\n"
          "    -reads file       instead of -readmers: count the read k-mers of this FASTA / FASTQ file (plain, .gz, .bz2, .xz) on\n"
          "                      the GPU into the k-mers the run asks for; repeatable.  -hist, -dump and the variant modes (k <= 31)\n"
          "    -k k              k when no database gives it (-reads without -seqmers); must agree with -seqmers\n"
          "    -convert db       no report: rewrite the k-mer database <db> (any accepted form) as -output <file> in the flat form\n"
          "                      (sorted k-mers in delta-coded blocks; loads at the speed of the PCIe link)\n"
          "    -count            no report: count every k-mer of the -reads files on the GPU (`meryl count`; -k K, K <= 31) and write\n"
          "                      the sorted flat database -output <file>, which every mode takes as -readmers.  -min / -max are not\n"
          "                      applied: a database holds every count, the filter acts when it is loaded.  One device.\n"
          "    -passes P|auto    with -count: the k-mers are counted in P passes (1 to 4096) over ascending key ranges, each in a table\n"
          "                      of its own, for read sets whose table does not fit the device (-memory); auto: one pass, and a range\n"
          "                      whose table cannot grow is cut in two.  The reads are parsed once and kept packed in host memory.\n"
          "    -placed           with -convert: the records sorted by their PLACE in the table -hist / -dump build (13 <= k <= 31,\n"
          "                      canonical databases): such a database is applied to the table line after line\n"
          "    -device d         HIP device (default 0)\n"
          "    -devices list     several GPUs of this node driven by this one process, e.g. 0-7 or 0,2,5 (-hist: the index is\n"
          "                      built once and copied to the others over xGMI, every GPU evaluates its share of the\n"
          "                      sequence, the histograms are added; -dump and the variant modes: every GPU takes a contiguous\n"
          "                      run of contigs, the outputs are concatenated in order; -completeness uses the first device)\n"
          "    -sharded          with -devices: every GPU keeps only its share of the k-mer table (read databases too large\n"
          "                      for one GPU).  -hist routes every k-mer to the GPU that owns it; -dump and the variant modes\n"
          "                      look every k-mer up in all shards and add the answers; -completeness adds per-shard sums\n"
          "    -index file       cache of the built HBM index: loaded if it exists (the k-mer databases are then not\n"
          "                      read), otherwise written after the build\n"
          "    -window W         with -track: k-mer start positions per window (default 1000)\n"
          "    -copies C         with -spectrum: rows for assembly counts 1 .. C, one more for > C (1 to 6, default 4)\n"
          "    -maxmult M        with -spectrum: read counts of M and more share the last column (4 to 65536, default 10000)\n\n"
          "  Report types (exactly one):\n"
          "    -hist           0-centred K* histogram to <output>; QV and QV* on stderr\n"
          "    -dump           seqName, seqPos, readK, asmK, K* per k-mer to <output>  [-skipMissing]\n"
          "    -completeness   k-mer completeness from -seqmers (or -sequence) and -readmers\n"
          "    -track          K* summarised per window of every contig on the GPU -> <output>.track.tsv, <output>.kstar.bedgraph\n"
          "                    (mean K*) and <output>.missing.bedgraph (missing fraction)  [-window W]; an <output> ending in\n"
          "                    .gz / .bz2 / .xz compresses the three files (out.gz -> out.track.tsv.gz ...)\n"
          "    -spectrum       copy-number spectrum (k-mers per read count and assembly count) -> <output>.spectra-cn.hist; the haploid\n"
          "                    peak it shows on stderr.  No -peak needed.  [-copies C] [-maxmult M]\n"
          "    -filter         keep variants (and combinations within k) that minimise missing k-mers -> <output>.filter.vcf\n"
          "    -polish         choose variant combinations by missing k-mers, ties by k* -> <output>.polish.vcf\n"
          "    -better -strict -loose   k*-free variants of -polish -> <output>.filter.vcf\n"
          "                    [-comb N (15)] [-nosplit] [-debug -> <output>.00.debug.gz]\n\n",
          exe);
}

// the entries of -merge and -op: printed behind the text above for a command line that names one of them
static void usage_merge() {
  fprintf(stderr,
          "  Merging k-mer databases (an operation of its own, like -count and -convert):\n"
          "    -merge db         no report: combine sorted flat databases (what -count and -convert write; one k) on the GPU, window by window,\n"
          "                      into the sorted flat database -output <file>; repeatable, 1 to 64 inputs (`meryl union-sum` and its kin).\n"
          "                      Here -min / -max ARE applied, to the combined count: one input and -min 2 drops the singletons.  One device.\n"
          "    -op o             with -merge: sum (default; saturating at 2^32 - 1), max, min (all three keep every k-mer of any input) or\n"
          "                      intersect (the k-mers every input holds, with their smallest count)\n"
          "\n");
}

// the entry of -not: printed behind the text above for a command line that names it
static void usage_not() {
  fprintf(stderr,
          "    -not db           with -merge: the k-mers of this sorted flat database are not written, whatever their counts there (`meryl\n"
          "                      difference`; hap-mers: -merge mat.mfxk -not pat.mfxk); repeatable; the -merge and -not databases are 64 at the most\n"
          "\n");
}

// the entry of -join: printed behind the text above for a command line that names it
static void usage_join() {
  fprintf(stderr,
          "  -completeness and -spectrum without a table:\n"
          "    -join             with -completeness and -spectrum: -readmers and -seqmers, both sorted flat databases (what -count and -convert\n"
          "                      write; one k <= 31), are joined on the GPU window by window, so neither has to fit the device.  An assembly's\n"
          "                      database is made by: merfin -count -reads asm.fasta -k K -output asm.mfxk.  -peak <number>, not auto.  One device.\n"
          "\n");
}

// the entries of -regions: printed behind the text above for a command line that names one of its flags
static void usage_regions() {
  fprintf(stderr,
          "  Intervals instead of windows (a report type, like -track):\n"
          "    -regions          maximal runs of missing (readK = 0), collapsed (K* >= t) and expanded (K* <= -t) k-mers of every contig, made on\n"
          "                      the GPU -> <output>.regions.bed: chrom, base span, class, flagged k-mers, mean readK, mean asmK, extreme K*.\n"
          "                      An <output> ending in .gz / .bz2 / .xz compresses it (out.gz -> out.regions.bed.gz).  One device.\n"
          "                      Takes -reads, -seqmers, -index and -peak auto as -track does.\n"
          "    -kstar t          with -regions: the threshold t, a finite number above 0 (default 1.0)\n"
          "    -gap g            with -regions: runs of one class and contig with at most g positions between them are one region (default 0)\n"
          "    -minrun m         with -regions: regions of fewer than m flagged k-mers are dropped, after the joining (default 1)\n"
          "\n");
}

// the entries of -phase: printed behind the text above for a command line that names one of its flags
static void usage_phase() {
  fprintf(stderr,
          "  Trio phasing (an operation of its own: no -readmers, no -peak):\n"
          "    -phase            hap-mer markers of two parents on every contig of -sequence, their phase blocks and switch errors, made on the\n"
          "                      GPU -> <output>.phased_block.bed (chrom, base span, hap A / B, markers of the block's own and of the other\n"
          "                      haplotype, runs of the other), <output>.hapmers.count (per contig: A markers, B markers, shared, k-mers) and\n"
          "                      <output>.phased_block.stats.  An <output> ending in .gz / .bz2 / .xz compresses them.  One device.\n"
          "                      The block rule is this program's own, in the spirit of Merqury's phase blocks; it is not validated against Merqury.\n"
          "    -hapmers db       with -phase, exactly twice: the k-mers specific to haplotype A, then to B (any database form; one k).\n"
          "                      -min / -max apply to the counts of both.\n"
          "    -switches S       with -phase: a run of the other haplotype of at most S markers ... (default 100)\n"
          "    -range R          ... that spans at most R bases is a switch error inside a block; a longer one ends the block (default 20000)\n"
          "\n");
}

// the entries of -bin: printed behind the text above for a command line that names one of its flags
static void usage_bin() {
  fprintf(stderr,
          "  Trio binning (an operation of its own: no -sequence, no -readmers, no -peak):\n"
          "    -bin              per read of the -reads files (FASTA / FASTQ, plain or .gz / .bz2 / .xz; repeatable) the k-mers found in hap-mer\n"
          "                      set A only, in B only and in both, counted on the GPU (k <= 31), and the read's class -> <output>.bin.tsv\n"
          "                      (read, length, kmers, A, B, shared, class A / B / U; one line per read in input order) and\n"
          "                      <output>.bin.stats (reads, bases and hits per class).  An <output> ending in .gz / .bz2 / .xz compresses\n"
          "                      them.  One device.  With NA, NB the k-mers of the two sets a read is A iff A + B >= m and\n"
          "                      A / NA > r * B / NB, B iff the same holds with the roles swapped, else U (unknown).  The rule is this\n"
          "                      program's own, in the spirit of Canu's haplotype split; it is not validated against Canu.\n"
          "    -hapmers db       with -bin, exactly twice: the k-mers specific to haplotype A, then to B (any database form; one k).\n"
          "                      -min / -max apply to the counts of both.\n"
          "    -ratio r          with -bin: the factor r, a decimal of at most three places, at least 1 (default 1.0)\n"
          "    -minhits m        with -bin: reads with fewer than m hits of either set are unknown (default 1)\n"
          "    -split            with -bin: the reads are written to <output>.hapA.fasta, <output>.hapB.fasta and <output>.unknown.fasta,\n"
          "                      name and bases as read; the reader drops the qualities of a FASTQ\n"
          "\n");
}

// the entries of -trio and -histogram: printed behind the text above for a command line that names one of their flags
static void usage_trio() {
  fprintf(stderr,
          "  Hap-mer databases of a trio, and k-mer histograms (operations of their own: no -sequence, no -readmers, no -peak):\n"
          "    -trio             the k-mers of -mat that -pat does not hold -> <output>.hapA.mfxk, those of -pat that -mat does not hold ->\n"
          "                      <output>.hapB.mfxk (what -phase and -bin take as -hapmers), each k-mer with a count of its cutoff or more;\n"
          "                      with -child only the k-mers the child holds, with the smaller of the two counts.  One windowed pass over the\n"
          "                      sorted flat databases (what -count and -convert write; one k <= 31) on the GPU, no intermediate file; the\n"
          "                      counters -> <output>.trio.stats.  One device.  The rule is this program's own, in the spirit of Merqury's\n"
          "                      hapmers.sh; it is not validated against Merqury.\n"
          "    -mat db / -pat db the parents' databases;  -child db  the child's (optional)\n"
          "    -cutmat n|auto    -cutpat, -cutchild likewise: the smallest count kept, 1 or more (k-mers below it are taken for sequencing\n"
          "                      errors); auto (the default): the first valley of the database's k-mer histogram, made on the GPU in a pass\n"
          "                      before -- of the k-mers the other parent does not hold for -mat and -pat -- and written to\n"
          "                      <output>.mat_only.hist, <output>.pat_only.hist and <output>.child.hist\n"
          "    -histogram db     the k-mer histogram of a sorted flat database (`meryl histogram`) -> -output <file>: count, k-mers per line,\n"
          "                      the form GenomeScope reads; valley and peaks on stderr.  An <output> ending in .gz / .bz2 / .xz is compressed.\n"
          "    -maxmult M        with -trio and -histogram: counts of M and more share the last line (4 to 65536, default 10000)\n"
          "\n");
}

// the entry of -diploid: printed behind the text above for a command line that names it or one of its flags
static void usage_diploid() {
  fprintf(stderr,
          "  Two haplotype assemblies against the reads (an operation of its own: no -sequence, no -seqmers):\n"
          "    -diploid          -readmers reads.mfxk -hap1 h1.mfxk -hap2 h2.mfxk -output stem: one windowed join of the three sorted flat\n"
          "                      databases (what -count and -convert write; one k <= 31) on the GPU, no table, no intermediate file; the read\n"
          "                      database is read once.  It writes <output>.spectra-asm.hist (the k-mers of the reads alone, of hap1 alone, of\n"
          "                      hap2 alone and of both, by read count), <output>.spectra-cn.hist (the file -spectrum -join writes for\n"
          "                      -merge hap1 hap2), <output>.qv (per hap1 / hap2 / both: the assembly's k-mers the reads do not hold, all of\n"
          "                      them, QV and error rate; a second block with the distinct counts) and <output>.completeness.stats (the solid\n"
          "                      read k-mers an assembly holds).  One device.  QV and completeness follow Merqury's in spirit; they are\n"
          "                      unvalidated against Merqury.\n"
          "    -hap1 db / -hap2 db  the assemblies' databases (merfin -count -reads hap1.fasta -k K -output h1.mfxk); they may be one file\n"
          "    -copies C / -maxmult M  the rows and columns of the two images (as -spectrum);  -min m / -max m  the read counts that count as\n"
          "                      present in the images and the completeness (the QV uses the raw read count)\n"
          "    -peak P [-prob t] also print merfin's -completeness report of hap1, of hap2 and of both (-peak auto is not taken: no table)\n"
          "\n");
}

// the usage text, then what is wrong with this command line; the exit code of a refused run
static int fail_usage(const char *argv0, const Errors &err, bool merge = false, bool join = false, bool regions = false, bool phase = false, bool nots = false,
                      bool bin = false, bool trio = false, bool diploid = false) {
  usage(argv0);
  if (merge) usage_merge();
  if (nots) usage_not();
  if (join) usage_join();
  if (regions) usage_regions();
  if (phase) usage_phase();
  if (bin) usage_bin();
  if (trio) usage_trio();
  if (diploid) usage_diploid();
  for (auto &e : err) fputs(e.c_str(), stderr);
  return 1;
}

// a knob of the environment that holds a number (docs/KNOBS.md): -1 when it is not set
static int env_flag(const char *name) {
  const char *e = getenv(name);
  return e ? atoi(e) : -1;
}

static bool variant_mode(int reportType) { return reportType >= OP_FILTER && reportType <= OP_LOOSE; }

// The integer arguments: decimal digits and nothing else, a minus sign in front at the most (which only ever says "below lo").
enum { UINT_OK, UINT_NOT_A_NUMBER, UINT_BELOW, UINT_ABOVE };
static int parse_uint(const char *v, unsigned long long lo, unsigned long long hi, unsigned long long *out) {
  const bool minus = v[0] == '-';
  char *e = nullptr;
  errno = 0;
  const unsigned long long x = strtoull(v + minus, &e, 10);
  if (!isdigit((unsigned char)v[minus]) || *e != 0 || errno != 0) return UINT_NOT_A_NUMBER;
  if (x < lo || (minus && x > 0)) return UINT_BELOW;
  if (x > hi) return UINT_ABOVE;
  *out = x;
  return UINT_OK;
}

// -ratio: digits, then at most a point and one to three digits; thousandths, 1000 to 4 000 000 000
static bool parse_milli(const char *v, uint32_t *out) {
  size_t i = 0;
  unsigned long long ip = 0;
  if (!isdigit((unsigned char)v[0])) return false;
  for (; isdigit((unsigned char)v[i]); ++i) {
    ip = ip * 10 + (unsigned long long)(v[i] - '0');
    if (ip > 4000000ull) return false;
  }
  unsigned long long fr = 0;
  if (v[i] == '.') {
    size_t d = 0;
    for (++i; isdigit((unsigned char)v[i]); ++i, ++d) fr = fr * 10 + (unsigned long long)(v[i] - '0');
    if (d == 0 || d > 3) return false;
    for (; d < 3; ++d) fr *= 10;
  }
  if (v[i] != 0 || ip < 1) return false;
  *out = (uint32_t)(ip * 1000 + fr);
  return true;
}

// -devices "0-7", "0,2,5", "0-3,6": a device may be named twice (two evaluation contexts on one GPU)
static bool parse_devices(const std::string &spec, std::vector<int> &devices) {
  bool ok = !spec.empty();
  for (size_t i = 0; ok && i < spec.size();) {
    char *e = nullptr;
    long a = strtol(spec.c_str() + i, &e, 10), b = a;
    ok = e != spec.c_str() + i && a >= 0;
    i = (size_t)(e - spec.c_str());
    if (ok && i < spec.size() && spec[i] == '-') {
      const char *s2 = spec.c_str() + i + 1;
      b = strtol(s2, &e, 10);
      ok = e != s2 && b >= a;
      i = (size_t)(e - spec.c_str());
    }
    for (long d = a; ok && d <= b && d < 1024; ++d) devices.push_back((int)d);
    if (ok && i < spec.size()) { ok = spec[i] == ','; ++i; }
  }
  if (!ok || devices.empty()) devices.clear();
  return !devices.empty();
}

static void parse_args(int argc, char **argv, Globals &G, Errors &err) {
  for (int arg = 1; arg < argc; arg++) {
    auto is = [&](const char *f) { return strcmp(argv[arg], f) == 0; };
    auto val = [&]() -> const char * { return arg + 1 < argc ? argv[++arg] : ""; };
    unsigned long long x = 0;
    if (is("-sequence")) G.seqName = val();
    else if (is("-seqmers")) G.seqDBname = val();
    else if (is("-readmers")) { G.readDBname = val(); ++G.readmersGiven; }
    else if (is("-diploid")) G.diploid = true;
    else if (is("-hap1")) G.hap1Names.push_back(val());
    else if (is("-hap2")) G.hap2Names.push_back(val());
    else if (is("-reads")) G.readsNames.push_back(val());
    else if (is("-k")) {
      const char *v = val();
      G.kArg = parse_uint(v, 1, 64, &x) == UINT_OK ? (int)x : -1;
      if (G.kArg < 0) err.push_back(std::string("Invalid -k '") + v + "': k is 1 to 64.\n");
    }
    else if (is("-peak")) {
      const char *v = val();
      if (strcmp(v, "auto") == 0) G.peakAuto = true;
      else G.peak = strtod(v, nullptr);
      G.peakGiven = true;
    }
    else if (is("-spectrum")) G.reportType = OP_SPECTRUM;
    else if (is("-copies") || is("-maxmult")) {
      const bool cp = is("-copies");
      const char *v = val();
      const unsigned long long lo = cp ? 1 : 4, hi = cp ? 6 : 65536;
      (cp ? G.copiesGiven : G.maxMultGiven) = true;
      if (parse_uint(v, lo, hi, &x) != UINT_OK)
        err.push_back(std::string("Invalid ") + (cp ? "-copies" : "-maxmult") + " '" + v + "': an integer from " + std::to_string(lo) + " to " + std::to_string(hi) + ".\n");
      else (cp ? G.copies : G.maxMult) = (uint32_t)x;
    }
    else if (is("-prob")) G.pLookupTable = val();
    else if (is("-vcf")) G.vcfName = val();
    else if (is("-output")) G.outName = val();
    else if (is("-min")) G.minV = strtoull(val(), nullptr, 10);
    else if (is("-max")) G.maxV = strtoull(val(), nullptr, 10);
    else if (is("-threads")) G.threads = atoi(val());
    else if (is("-memory")) G.maxMemory = strtod(val(), nullptr);
    else if (is("-device")) G.device = atoi(val());
    else if (is("-devices")) {
      const std::string spec = val();
      if (!parse_devices(spec, G.devices)) err.push_back(std::string("Invalid device list '") + spec + "' (-devices 0-7 or 0,2,5).\n");
    }
    else if (is("-index")) G.indexName = val();
    else if (is("-sharded")) G.sharded = true;
    else if (is("-convert")) G.convertName = val();
    else if (is("-count")) G.count = true;
    else if (is("-merge")) G.mergeNames.push_back(val());
    else if (is("-not")) G.notNames.push_back(val());
    else if (is("-join")) G.join = true;
    else if (is("-op")) {
      G.opName = val();
      static const char *const names[] = {"sum", "max", "min", "intersect"};      // MFX_MERGE_*
      int op = -1;
      for (int i = 0; i < 4; ++i) if (strcmp(G.opName, names[i]) == 0) op = i;
      if (op < 0) err.push_back(std::string("Invalid -op '") + G.opName + "': the operations of -merge are sum, max, min and intersect.\n");
      else G.mergeOp = op;
    }
    else if (is("-passes")) {
      const char *v = val();
      const int bad = strcmp(v, "auto") == 0 ? UINT_OK : parse_uint(v, 1, 4096, &x);
      G.passesGiven = true;
      if (strcmp(v, "auto") == 0) G.passesAuto = true;
      else if (bad == UINT_NOT_A_NUMBER) err.push_back(std::string("Invalid -passes '") + v + "': the passes of -count are a number from 1 to 4096, or auto.\n");
      else if (bad == UINT_BELOW) err.push_back(std::string("Invalid -passes '") + v + "': -count takes at least one pass (1 to 4096, or auto).\n");
      else if (bad == UINT_ABOVE) err.push_back(std::string("Invalid -passes '") + v + "': a pass takes at least one of the 4096 key bins, so there are 4096 at most (or auto).\n");
      else G.passes = (uint32_t)x;
    }
    else if (is("-placed")) G.placed = true;
    else if (is("-nosplit")) G.nosplit = true;
    else if (is("-filter")) G.reportType = OP_FILTER;
    else if (is("-better")) G.reportType = OP_BETTER;
    else if (is("-strict")) G.reportType = OP_STRICT;
    else if (is("-loose")) { fprintf(stderr, "*EXPERIMENTAL* Running in -loose mode\n"); G.reportType = OP_LOOSE; }
    else if (is("-polish")) G.reportType = OP_POLISH;
    else if (is("-hist")) G.reportType = OP_HIST;
    else if (is("-dump")) G.reportType = OP_DUMP;
    else if (is("-track")) G.reportType = OP_TRACK;
    else if (is("-window")) {
      const char *v = val();
      G.windowGiven = true;
      if (parse_uint(v, 1, ~0ull, &x) != UINT_OK) err.push_back(std::string("Invalid -window '") + v + "': a window is an integer of at least 1.\n");
      else G.window = x;
    }
    else if (is("-regions")) G.reportType = OP_REGIONS;
    else if (is("-kstar")) {
      const char *v = val();
      char *e = nullptr;
      G.kstarGiven = true;
      errno = 0;
      const double t = strtod(v, &e);
      if (e == v || *e != 0 || isspace((unsigned char)v[0]) || !(t > 0) || !(t <= 1.7976931348623157e308))
        err.push_back(std::string("Invalid -kstar '") + v + "': the threshold of -regions is a finite number above 0.\n");
      else G.regKstar = t;
    }
    else if (is("-gap") || is("-minrun")) {
      const bool gp = is("-gap");
      const char *v = val();
      (gp ? G.gapGiven : G.minrunGiven) = true;
      if (parse_uint(v, 0, ~0ull, &x) != UINT_OK)
        err.push_back(std::string("Invalid ") + (gp ? "-gap" : "-minrun") + " '" + v + "': " + (gp ? "a gap is a number of positions" : "-minrun is a number of k-mers") + ", an integer of at least 0.\n");
      else (gp ? G.regGap : G.regMinrun) = x;
    }
    else if (is("-phase")) G.phase = true;
    else if (is("-hapmers")) G.hapmers.push_back(val());
    else if (is("-switches") || is("-range")) {
      const bool sw = is("-switches");
      const char *v = val();
      (sw ? G.switchesGiven : G.rangeGiven) = true;
      if (parse_uint(v, 0, ~0ull, &x) != UINT_OK)
        err.push_back(std::string("Invalid ") + (sw ? "-switches" : "-range") + " '" + v + "': " + (sw ? "-switches is a number of markers" : "-range is a number of bases") + ", an integer of at least 0.\n");
      else (sw ? G.phSwitches : G.phRange) = x;
    }
    else if (is("-bin")) G.bin = true;
    else if (is("-split")) G.binSplit = true;
    else if (is("-ratio")) {
      const char *v = val();
      G.ratioGiven = true;
      if (!parse_milli(v, &G.binRatioMilli))
        err.push_back(std::string("Invalid -ratio '") + v + "': the ratio of -bin is a decimal of at most three places, 1 to 4000000.\n");
    }
    else if (is("-minhits")) {
      const char *v = val();
      G.minhitsGiven = true;
      if (parse_uint(v, 0, 0xffffffffull, &x) != UINT_OK) err.push_back(std::string("Invalid -minhits '") + v + "': -minhits is a number of k-mers, an integer from 0 to 4294967295.\n");
      else G.binMinHits = (uint32_t)x;
    }
    else if (is("-trio")) G.trio = true;
    else if (is("-mat")) G.matName = val();
    else if (is("-pat")) G.patName = val();
    else if (is("-child")) G.childName = val();
    else if (is("-histogram")) G.histName = val();
    else if (is("-cutmat") || is("-cutpat") || is("-cutchild")) {
      const std::string flag = argv[arg];
      const int which = flag == "-cutmat" ? 0 : flag == "-cutpat" ? 1 : 2;
      const char *v = val();
      (which == 0 ? G.cutMatGiven : which == 1 ? G.cutPatGiven : G.cutChildGiven) = true;
      uint32_t &cut = which == 0 ? G.cutMat : which == 1 ? G.cutPat : G.cutChild;
      if (strcmp(v, "auto") == 0) cut = 0;
      else if (parse_uint(v, 1, 0xffffffffull, &x) != UINT_OK)
        err.push_back("Invalid " + flag + " '" + v + "': a cutoff of -trio is a count from 1 to 4294967295, or auto.\n");
      else cut = (uint32_t)x;
    }
    else if (is("-skipMissing")) G.skipMissing = true;
    else if (is("-completeness")) G.reportType = OP_COMPL;
    else if (is("-comb")) G.comb = (unsigned)strtoul(val(), nullptr, 10);
    else if (is("-debug")) G.debug = true;
    else err.push_back(std::string("Unknown option '") + argv[arg] + "'.\n");
  }
}

// can every -reads file be read?  One line per file that cannot
static void reads_files_readable(const Globals &G, Errors &err) {
  for (const char *f : G.readsNames) {
    struct stat rst;
    if (stat(f, &rst) != 0 || !S_ISREG(rst.st_mode) || access(f, R_OK) != 0)
      err.push_back(std::string("Cannot read the -reads file '") + f + "'.\n");
  }
}

// false, with the reference's text: a device of the run is not there.  (Stays on the main thread, before anything else is started: the HIP
// runtime coming up on a thread of its own while this one spawns a decompressor for -sequence was seen to come up with no device.)
static bool devices_available(const std::vector<int> &devs) {
  for (int d : devs)
    if (mfx_device_count() <= d) {
      fprintf(stderr, "ERROR: HIP device %d not available (%d visible). This program has no CPU path.\n", d, mfx_device_count());
      return false;
    }
  return true;
}

// -merge: every check before any device is touched (what the inputs hold is checked by mfx_db_merge, before it touches one)
static void check_merge_flags(const Globals &G, Errors &err) {
  if (G.mergeNames.empty()) {
    if (G.opName) err.push_back("-op names the operation of -merge: it has no meaning without -merge.\n");
    if (!G.notNames.empty()) err.push_back("-not names a database to subtract in -merge: it has no meaning without -merge.\n");
    return;
  }
  if (G.reportType != OP_NONE) err.push_back("-merge is an operation of its own: it does not take a report type (-hist, -dump, -completeness, ...).\n");
  if (G.count) err.push_back("-merge and -count are two operations: give one of them.\n");
  if (G.convertName) err.push_back("-merge and -convert are two operations: give one of them.\n");
  if (!G.readsNames.empty()) err.push_back("-merge combines databases: it does not take -reads (count them first: -count).\n");
  if (G.readDBname) err.push_back("-merge takes its databases as -merge <file>: it does not take -readmers.\n");
  if (G.seqDBname) err.push_back("-merge takes its databases as -merge <file>: it does not take -seqmers.\n");
  if (G.seqName) err.push_back("-merge evaluates nothing: it does not take -sequence.\n");
  if (G.vcfName) err.push_back("-merge does not take -vcf (the variant modes do).\n");
  if (G.peakGiven) err.push_back("-merge evaluates nothing: it does not take -peak.\n");
  if (G.sharded) err.push_back("-merge does not take -sharded: the windows it merges live on one device.\n");
  if (G.indexName) err.push_back("-merge does not take -index: it writes a database, not a table image.\n");
  if (G.placed) err.push_back("-merge writes k-mer-sorted databases: it does not take -placed (convert the result: -convert -placed).\n");
  if (G.passesGiven) err.push_back("-passes divides the work of -count: -merge does not take it (MFX_MERGE_RANGE sizes its windows).\n");
  if (G.devices.size() > 1) err.push_back("-merge runs on one device (-device d, or -devices naming one).\n");
  if (!G.outName) err.push_back("-merge writes a k-mer database: give -output <file>.\n");
  if (G.mergeNames.size() > 64) err.push_back("-merge takes 1 to 64 databases (here " + std::to_string(G.mergeNames.size()) + "): merge them in groups.\n");
  for (const char *f : G.mergeNames) {
    struct stat mst;
    if (stat(f, &mst) != 0 || access(f, R_OK) != 0) err.push_back(std::string("Cannot read the -merge database '") + f + "'.\n");
  }
  if (!G.notNames.empty() && G.mergeNames.size() <= 64 && G.mergeNames.size() + G.notNames.size() > 64)
    err.push_back("-merge and -not take 64 databases at the most (here " + std::to_string(G.mergeNames.size()) + " and " + std::to_string(G.notNames.size()) + ").\n");
  for (const char *f : G.notNames) {
    struct stat mst;
    if (stat(f, &mst) != 0 || access(f, R_OK) != 0) err.push_back(std::string("Cannot read the -not database '") + f + "'.\n");
  }
}

// -count: every check before any device is touched (the checks of a report from -reads below do not apply to it)
static void check_count_flags(const Globals &G, Errors &err) {
  if (!G.count) {
    if (G.passesGiven) err.push_back("-passes divides the work of -count: it has no meaning without -count.\n");
    return;
  }
  if (G.convertName) err.push_back("-count and -convert are two operations: give one of them.\n");
  if (G.reportType != OP_NONE) err.push_back("-count is an operation of its own: it does not take a report type (-hist, -dump, -completeness, ...).\n");
  if (G.readsNames.empty()) err.push_back("-count needs the reads it counts: give -reads <file> (repeatable).\n");
  if (G.kArg == 0) err.push_back("-count needs -k: no database gives it.\n");
  if (!G.outName) err.push_back("-count writes a k-mer database: give -output <file>.\n");
  if (G.kArg > 31)
    err.push_back("-count holds k <= 31 (here k = " + std::to_string(G.kArg) + "): count larger k-mers with `meryl count` and give the database as -readmers.\n");
  if (G.readDBname) err.push_back("-count makes the read database: it does not take -readmers.\n");
  if (G.seqDBname) err.push_back("-count counts reads: it does not take -seqmers.\n");
  if (G.seqName) err.push_back("-count counts reads: it does not take -sequence.\n");
  if (G.vcfName) err.push_back("-count does not take -vcf (the variant modes do).\n");
  if (G.peakGiven) err.push_back("-count evaluates nothing: it does not take -peak.\n");
  if (G.sharded) err.push_back("-count does not take -sharded: the table it counts into lives on one device.\n");
  if (G.indexName) err.push_back("-count does not take -index: it writes a database, not a table image.\n");
  if (G.devices.size() > 1) err.push_back("-count runs on one device (-device d, or -devices naming one).\n");
  reads_files_readable(G, err);
}

// -reads: every check before any device is touched; G.kArg becomes the run's k.  false: -seqmers could not be opened (the error is printed)
static bool check_reads_flags(Globals &G, Errors &err) {
  const bool variants = variant_mode(G.reportType);
  if (!G.readsNames.empty()) {
    if (G.convertName) err.push_back("-convert rewrites a k-mer database; it does not take -reads.\n");
    if (G.readDBname) err.push_back("-reads and -readmers cannot be combined: the read counts come from one source.\n");
    if (G.reportType == OP_COMPL) err.push_back("-completeness needs every read k-mer: it takes a read database (-readmers), not -reads.\n");
    if (G.sharded) err.push_back("-sharded does not take -reads (give the read database with -readmers).\n");
    if (G.kArg == 0 && !G.seqDBname) err.push_back("-reads needs -k (or -seqmers, whose k it then takes).\n");
    reads_files_readable(G, err);
    if (variants && (G.indexName || G.devices.size() > 1))
      err.push_back("The variant modes count -reads into the path-only index of the call set: one device, no -index.\n");
    if (G.seqDBname && !G.convertName && !G.readDBname) {
      mfx_db_info sdb;
      if (mfx_db_probe(G.seqDBname, &sdb)) { fprintf(stderr, "ERROR: %s: %s\n", "opening -seqmers", mfx_last_error()); return false; }
      if (G.kArg > 0 && sdb.k != G.kArg) err.push_back("-k " + std::to_string(G.kArg) + " disagrees with -seqmers, which holds " + std::to_string(sdb.k) + "-mers.\n");
      else G.kArg = sdb.k;
    }
    if (variants && G.kArg > 31)
      err.push_back("The variant modes count -reads into the path-only index, which holds k <= 31 (here k = " + std::to_string(G.kArg) + ").\n");
  }
  if (G.kArg > 0 && G.readDBname && G.readsNames.empty()) err.push_back("-k is taken from -readmers; give -k only with -reads.\n");
  return true;
}

// -track: every check before any device is touched
static void check_track_flags(const Globals &G, Errors &err) {
  if (G.windowGiven && G.reportType != OP_TRACK) err.push_back("-window sets the window of -track; it has no meaning without -track.\n");
  if (G.reportType != OP_TRACK) return;
  if (G.sharded) err.push_back("-track does not take -sharded: a window's records need every k-mer's counts on one device.\n");
  if (G.devices.size() > 1) err.push_back("-track runs on one device (-device d, or -devices naming one).\n");
  if (G.skipMissing) err.push_back("-skipMissing belongs to -dump; -track always writes its windows.\n");
  if (G.vcfName) err.push_back("-track does not take -vcf (the variant modes do).\n");
}

// -regions: every check before any device is touched
static bool regions_named(const Globals &G) { return G.reportType == OP_REGIONS || G.kstarGiven || G.gapGiven || G.minrunGiven; }
static void check_regions_flags(const Globals &G, Errors &err) {
  if (G.reportType != OP_REGIONS) {
    if (G.kstarGiven) err.push_back("-kstar sets the threshold of -regions; it has no meaning without -regions.\n");
    if (G.gapGiven) err.push_back("-gap joins the runs of -regions; it has no meaning without -regions.\n");
    if (G.minrunGiven) err.push_back("-minrun drops short regions of -regions; it has no meaning without -regions.\n");
    return;
  }
  if (G.sharded) err.push_back("-regions does not take -sharded: a k-mer's class needs its whole counts on one device.\n");
  if (G.devices.size() > 1) err.push_back("-regions runs on one device (-device d, or -devices naming one).\n");
  if (G.skipMissing) err.push_back("-skipMissing belongs to -dump; -regions writes the missing k-mers as intervals.\n");
  if (G.vcfName) err.push_back("-regions does not take -vcf (the variant modes do).\n");
}

// -phase: every check before any device is touched (the two databases are probed on the host for their k)
static bool phase_named(const Globals &G) { return G.phase || !G.hapmers.empty() || G.switchesGiven || G.rangeGiven; }
static void check_phase_flags(const Globals &G, Errors &err) {
  if (!G.phase) {
    if (!G.hapmers.empty()) err.push_back("-hapmers names a hap-mer database of -phase; it has no meaning without -phase.\n");
    if (G.switchesGiven) err.push_back("-switches bounds the switch errors of -phase; it has no meaning without -phase.\n");
    if (G.rangeGiven) err.push_back("-range bounds the switch errors of -phase; it has no meaning without -phase.\n");
    return;
  }
  if (G.hapmers.size() != 2) err.push_back("-phase takes exactly two -hapmers databases, haplotype A then B (here " + std::to_string(G.hapmers.size()) + ").\n");
  if (G.reportType != OP_NONE) err.push_back("-phase is an operation of its own: it does not take a report type (-hist, -dump, -completeness, ...).\n");
  if (G.count || G.convertName || !G.mergeNames.empty()) err.push_back("-phase, -count, -convert and -merge are separate operations: give one of them.\n");
  if (G.readDBname) err.push_back("-phase takes its k-mers as -hapmers <file>: it does not take -readmers.\n");
  if (G.seqDBname) err.push_back("-phase does not count the assembly's k-mers: it does not take -seqmers.\n");
  if (!G.readsNames.empty()) err.push_back("-phase takes databases of hap-mers: it does not take -reads (count them first: -count).\n");
  if (G.peakGiven) err.push_back("-phase evaluates no K*: it does not take -peak.\n");
  if (G.pLookupTable) err.push_back("-phase evaluates no K*: it does not take -prob.\n");
  if (G.vcfName) err.push_back("-phase does not take -vcf (the variant modes do).\n");
  if (G.sharded) err.push_back("-phase does not take -sharded: a marker needs both sets' whole membership on one device.\n");
  if (G.devices.size() > 1) err.push_back("-phase runs on one device (-device d, or -devices naming one).\n");
  if (G.indexName) err.push_back("-phase does not take -index: its table holds the two hap-mer sets, not a run's counts.\n");
  if (G.join) err.push_back("-join is a way to run -completeness and -spectrum: -phase does not take it.\n");
  if (!G.seqName) err.push_back("No input sequences (-sequence) supplied.\n");
  if (!G.outName) err.push_back("No output (-output) supplied.\n");
  if (G.hapmers.size() == 2) {
    if (strcmp(G.hapmers[0], G.hapmers[1]) == 0) {
      err.push_back(std::string("-phase needs two different hap-mer sets: both -hapmers name '") + G.hapmers[0] + "'.\n");
    } else {
      mfx_db_info a, b;
      const bool oka = mfx_db_probe(G.hapmers[0], &a) == MFX_OK;
      if (!oka) err.push_back(std::string("Cannot open the -hapmers database '") + G.hapmers[0] + "': " + mfx_last_error() + "\n");
      const bool okb = mfx_db_probe(G.hapmers[1], &b) == MFX_OK;
      if (!okb) err.push_back(std::string("Cannot open the -hapmers database '") + G.hapmers[1] + "': " + mfx_last_error() + "\n");
      if (oka && okb && a.k != b.k)
        err.push_back("The two -hapmers databases hold different k-mers: " + std::to_string(a.k) + "-mers and " + std::to_string(b.k) + "-mers.\n");
    }
  }
}

// -bin: every check before any device is touched (the two databases are probed on the host for their k)
static bool bin_named(const Globals &G) { return G.bin || G.ratioGiven || G.minhitsGiven || G.binSplit; }
static void check_bin_flags(const Globals &G, Errors &err) {
  if (!G.bin) {
    if (G.ratioGiven) err.push_back("-ratio sets the class rule of -bin; it has no meaning without -bin.\n");
    if (G.minhitsGiven) err.push_back("-minhits sets the class rule of -bin; it has no meaning without -bin.\n");
    if (G.binSplit) err.push_back("-split writes the reads of -bin per class; it has no meaning without -bin.\n");
    return;
  }
  if (G.hapmers.size() != 2) err.push_back("-bin takes exactly two -hapmers databases, haplotype A then B (here " + std::to_string(G.hapmers.size()) + ").\n");
  if (G.reportType != OP_NONE) err.push_back("-bin is an operation of its own: it does not take a report type (-hist, -dump, -completeness, ...).\n");
  if (G.count || G.convertName || !G.mergeNames.empty() || G.phase) err.push_back("-bin, -phase, -count, -convert and -merge are separate operations: give one of them.\n");
  if (G.readsNames.empty()) err.push_back("-bin needs the reads it sorts: give -reads <file> (repeatable).\n");
  if (G.seqName) err.push_back("-bin sorts reads, it evaluates no assembly: it does not take -sequence (-phase does).\n");
  if (G.readDBname) err.push_back("-bin takes its k-mers as -hapmers <file>: it does not take -readmers.\n");
  if (G.seqDBname) err.push_back("-bin takes its k-mers as -hapmers <file>: it does not take -seqmers.\n");
  if (G.peakGiven) err.push_back("-bin evaluates no K*: it does not take -peak.\n");
  if (G.pLookupTable) err.push_back("-bin evaluates no K*: it does not take -prob.\n");
  if (G.vcfName) err.push_back("-bin does not take -vcf (the variant modes do).\n");
  if (G.sharded) err.push_back("-bin does not take -sharded: a read's counts need both sets' whole membership on one device.\n");
  if (G.devices.size() > 1) err.push_back("-bin runs on one device (-device d, or -devices naming one).\n");
  if (G.indexName) err.push_back("-bin does not take -index: its table holds the two hap-mer sets, not a run's counts.\n");
  if (G.join) err.push_back("-join is a way to run -completeness and -spectrum: -bin does not take it.\n");
  if (G.switchesGiven || G.rangeGiven) err.push_back("-switches and -range bound the switch errors of -phase: -bin does not take them.\n");
  if (!G.outName) err.push_back("No output (-output) supplied.\n");
  reads_files_readable(G, err);
  if (G.hapmers.size() == 2) {
    if (strcmp(G.hapmers[0], G.hapmers[1]) == 0) {
      err.push_back(std::string("-bin needs two different hap-mer sets: both -hapmers name '") + G.hapmers[0] + "'.\n");
    } else {
      mfx_db_info a, b;
      const bool oka = mfx_db_probe(G.hapmers[0], &a) == MFX_OK;
      if (!oka) err.push_back(std::string("Cannot open the -hapmers database '") + G.hapmers[0] + "': " + mfx_last_error() + "\n");
      const bool okb = mfx_db_probe(G.hapmers[1], &b) == MFX_OK;
      if (!okb) err.push_back(std::string("Cannot open the -hapmers database '") + G.hapmers[1] + "': " + mfx_last_error() + "\n");
      if (oka && okb && a.k != b.k)
        err.push_back("The two -hapmers databases hold different k-mers: " + std::to_string(a.k) + "-mers and " + std::to_string(b.k) + "-mers.\n");
      else if (oka && okb && a.k > 31)
        err.push_back("-bin holds k <= 31 (here k = " + std::to_string(a.k) + "): hap-mer databases of larger k-mers are not binned.\n");
      if (oka && okb && G.kArg > 0 && G.kArg != a.k) err.push_back("-k " + std::to_string(G.kArg) + " disagrees with -hapmers, which hold " + std::to_string(a.k) + "-mers.\n");
    }
  }
}

// -trio and -histogram: every check before any device is touched (what the databases hold is checked by mfx_db_trio / mfx_db_histogram,
// before they touch one)
static bool trio_named(const Globals &G) {
  return G.trio || G.matName || G.patName || G.childName || G.cutMatGiven || G.cutPatGiven || G.cutChildGiven || G.histName;
}
static void check_trio_flags(const Globals &G, Errors &err) {
  if (!trio_named(G)) return;
  const char *me = G.trio || !G.histName ? "-trio" : "-histogram";
  if (G.trio && G.histName) err.push_back("-trio and -histogram are two operations: give one of them.\n");
  if (!G.trio && !G.histName) {
    if (G.matName) err.push_back("-mat names the maternal database of -trio; it has no meaning without -trio.\n");
    if (G.patName) err.push_back("-pat names the paternal database of -trio; it has no meaning without -trio.\n");
    if (G.childName) err.push_back("-child names the child's database of -trio; it has no meaning without -trio.\n");
    if (G.cutMatGiven || G.cutPatGiven || G.cutChildGiven) err.push_back("-cutmat, -cutpat and -cutchild set the cutoffs of -trio; they have no meaning without -trio.\n");
    return;
  }
  if (G.reportType != OP_NONE) err.push_back(std::string(me) + " is an operation of its own: it does not take a report type (-hist, -dump, -completeness, -spectrum, ...).\n");
  if (G.count || G.convertName || !G.mergeNames.empty() || G.phase || G.bin)
    err.push_back(std::string(me) + ", -bin, -phase, -count, -convert and -merge are separate operations: give one of them.\n");
  if (G.join) err.push_back(std::string("-join is a way to run -completeness and -spectrum: ") + me + " does not take it.\n");
  if (G.readDBname) err.push_back(std::string(me) + " takes its databases by flags of its own: it does not take -readmers.\n");
  if (G.seqDBname) err.push_back(std::string(me) + " takes its databases by flags of its own: it does not take -seqmers.\n");
  if (G.seqName) err.push_back(std::string(me) + " evaluates nothing: it does not take -sequence.\n");
  if (!G.readsNames.empty()) err.push_back(std::string(me) + " reads databases: it does not take -reads (count them first: -count).\n");
  if (G.peakGiven) err.push_back(std::string(me) + " evaluates no K*: it does not take -peak.\n");
  if (G.vcfName) err.push_back(std::string(me) + " does not take -vcf (the variant modes do).\n");
  if (G.sharded) err.push_back(std::string(me) + " does not take -sharded: the windows it reads live on one device.\n");
  if (G.indexName) err.push_back(std::string(me) + " does not take -index: it builds no table.\n");
  if (G.copiesGiven) err.push_back(std::string("-copies shapes the image of -spectrum: ") + me + " does not take it.\n");
  if (G.devices.size() > 1) err.push_back(std::string(me) + " runs on one device (-device d, or -devices naming one).\n");
  if (G.trio) {
    if (!G.matName) err.push_back("-trio needs the maternal database: give -mat <file>.\n");
    if (!G.patName) err.push_back("-trio needs the paternal database: give -pat <file>.\n");
    if (!G.outName) err.push_back("-trio writes <output>.hapA.mfxk and <output>.hapB.mfxk: give -output <stem>.\n");
    if (G.cutChildGiven && !G.childName) err.push_back("-cutchild sets the cutoff of the child's database: it has no meaning without -child.\n");
    const char *const names[3] = {G.matName, G.patName, G.childName};
    const char *const flags[3] = {"-mat", "-pat", "-child"};
    for (int i = 0; i < 3; ++i) {
      struct stat mst;
      if (names[i] && (stat(names[i], &mst) != 0 || access(names[i], R_OK) != 0)) err.push_back(std::string("Cannot read the ") + flags[i] + " database '" + names[i] + "'.\n");
    }
  } else {
    if (G.matName || G.patName || G.childName || G.cutMatGiven || G.cutPatGiven || G.cutChildGiven)
      err.push_back("-mat, -pat, -child and the cutoffs belong to -trio: -histogram takes one database, -histogram <file>.\n");
    if (!G.outName) err.push_back("-histogram writes a k-mer histogram: give -output <file>.\n");
    struct stat mst;
    if (stat(G.histName, &mst) != 0 || access(G.histName, R_OK) != 0) err.push_back(std::string("Cannot read the -histogram database '") + G.histName + "'.\n");
  }
}

// -diploid: every check before any device is touched (what the databases hold is checked by mfx_db_diploid, before it touches one)
static bool diploid_named(const Globals &G) { return G.diploid || !G.hap1Names.empty() || !G.hap2Names.empty(); }
static void check_diploid_flags(const Globals &G, Errors &err) {
  if (!diploid_named(G)) return;
  if (!G.diploid) {
    err.push_back("-hap1 and -hap2 name the assemblies of -diploid; they have no meaning without -diploid.\n");
    return;
  }
  if (G.reportType != OP_NONE) err.push_back("-diploid is an operation of its own: it does not take a report type (-hist, -dump, -completeness, -spectrum, ...).\n");
  if (G.count || G.convertName || !G.mergeNames.empty() || G.phase || G.bin || G.trio || G.histName)
    err.push_back("-diploid, -trio, -histogram, -bin, -phase, -count, -convert and -merge are separate operations: give one of them.\n");
  if (G.join) err.push_back("-join is a way to run -completeness and -spectrum: -diploid is a join already and does not take it.\n");
  if (G.readmersGiven != 1) err.push_back(G.readmersGiven ? "-diploid takes one read database: -readmers was given more than once.\n" : "-diploid needs the read database: give -readmers <file>.\n");
  if (G.hap1Names.size() != 1) err.push_back(G.hap1Names.empty() ? "-diploid needs the first assembly's database: give -hap1 <file>.\n" : "-diploid takes two assemblies: -hap1 was given more than once.\n");
  if (G.hap2Names.size() != 1) err.push_back(G.hap2Names.empty() ? "-diploid needs the second assembly's database: give -hap2 <file>.\n" : "-diploid takes two assemblies: -hap2 was given more than once.\n");
  if (!G.outName) err.push_back("-diploid writes <output>.spectra-asm.hist, .spectra-cn.hist, .qv and .completeness.stats: give -output <stem>.\n");
  if (G.seqName) err.push_back("-diploid joins databases: it does not take -sequence (merfin -count -reads hap1.fasta -k K -output h1.mfxk, then -hap1 h1.mfxk).\n");
  if (G.seqDBname) err.push_back("-diploid takes its assemblies as -hap1 and -hap2: it does not take -seqmers.\n");
  if (!G.readsNames.empty()) err.push_back("-diploid joins databases: it does not take -reads (count them first: -count).\n");
  if (!G.hapmers.empty()) err.push_back("-diploid compares assemblies with the reads: it does not take -hapmers (-phase and -bin do).\n");
  if (!G.devices.empty()) err.push_back("-diploid runs on one device: it does not take -devices (-device d).\n");
  if (G.peakAuto) err.push_back("-diploid does not take -peak auto: the peak is read off a table, and -diploid builds none; give -peak <number>.\n");
  if (G.pLookupTable && !G.peakGiven) err.push_back("-prob belongs to the completeness report of -peak: give -peak <number> with it.\n");
  if (G.vcfName) err.push_back("-diploid does not take -vcf (the variant modes do).\n");
  if (G.sharded) err.push_back("-diploid does not take -sharded: the windows it joins live on one device, and no table is built.\n");
  if (G.indexName) err.push_back("-diploid does not take -index: it builds no table.\n");
  const char *const names[3] = {G.readmersGiven == 1 ? G.readDBname : nullptr, G.hap1Names.size() == 1 ? G.hap1Names[0] : nullptr, G.hap2Names.size() == 1 ? G.hap2Names[0] : nullptr};
  const char *const flags[3] = {"-readmers", "-hap1", "-hap2"};
  for (int i = 0; i < 3; ++i) {
    struct stat mst;
    if (names[i] && (stat(names[i], &mst) != 0 || access(names[i], R_OK) != 0)) err.push_back(std::string("Cannot read the ") + flags[i] + " database '" + names[i] + "'.\n");
  }
}

// -spectrum: every check before any device is touched
static void check_spectrum_flags(const Globals &G, Errors &err) {
  if ((G.copiesGiven || G.maxMultGiven) && G.reportType != OP_SPECTRUM)
    err.push_back("-copies and -maxmult shape the image of -spectrum; they have no meaning without -spectrum.\n");
  if (G.reportType != OP_SPECTRUM) return;
  if (G.vcfName) err.push_back("-spectrum does not take -vcf (the variant modes do).\n");
  if (G.sharded) err.push_back("-spectrum does not take -sharded: this version counts the spectrum of one table on one device.\n");
  if (G.devices.size() > 1) err.push_back("-spectrum runs on one device (-device d, or -devices naming one).\n");
  if (G.skipMissing) err.push_back("-skipMissing belongs to -dump; -spectrum counts every entry of the table.\n");
  if (!G.seqName && !G.seqDBname) err.push_back("No sequence meryl database (-seqmers) nor sequence (-sequence) supplied.\n");
  if (!G.seqName && !G.readsNames.empty()) err.push_back("-spectrum counts -reads into the k-mers of -sequence: give -sequence.\n");
}

// -join: every check before any device is touched (what the databases hold is checked by mfx_db_join_*, before it touches one)
static void check_join_flags(const Globals &G, Errors &err) {
  if (!G.join) return;
  if (G.reportType != OP_COMPL && G.reportType != OP_SPECTRUM)
    err.push_back("-join is a way to run -completeness and -spectrum: it does not take another report type (-hist, -dump, -track, the variant modes).\n");
  if (!G.readsNames.empty()) err.push_back("-join joins two databases: it does not take -reads (count them first: -count).\n");
  if (!G.seqDBname)
    err.push_back(G.seqName ? "-join joins two databases: it takes the assembly as -seqmers, not as -sequence (merfin -count -reads asm.fasta -k K -output asm.mfxk).\n"
                            : "-join joins two databases: give the assembly's as -seqmers (merfin -count -reads asm.fasta -k K -output asm.mfxk).\n");
  if (G.sharded) err.push_back("-join does not take -sharded: the windows it joins live on one device, and no table is built.\n");
  if (G.devices.size() > 1) err.push_back("-join runs on one device (-device d, or -devices naming one).\n");
  if (G.indexName) err.push_back("-join does not take -index: it builds no table.\n");
  if (G.peakAuto) err.push_back("-join does not take -peak auto: the peak is read off a table; give -peak <number>.\n");
}

// -peak auto: every check before any device is touched
static void check_peak_auto_flags(const Globals &G, Errors &err) {
  if (!G.peakAuto) return;
  if (G.peak != 0) err.push_back("-peak was given twice (a number and auto).\n");
  if (G.reportType != OP_HIST && G.reportType != OP_DUMP && G.reportType != OP_TRACK && G.reportType != OP_SPECTRUM && G.reportType != OP_REGIONS && G.reportType != OP_NONE)
    err.push_back("-peak auto reads the peak off the table of -hist, -dump, -track or -spectrum; the variant modes and -completeness take -peak <number>.\n");
  if (G.sharded) err.push_back("-peak auto does not take -sharded: no peak is defined on a sharded table.\n");
  if (G.devices.size() > 1) err.push_back("-peak auto runs on one device (-device d, or -devices naming one).\n");
}

// what every report needs, merfin.C:159-181
static void check_report_flags(const Globals &G, Errors &err) {
  if (G.reportType == OP_SPECTRUM) {
    if (!G.outName) err.push_back("No output (-output) supplied.\n");
  } else if (G.reportType != OP_COMPL) {
    if (!G.seqName) err.push_back("No input sequences (-sequence) supplied.\n");
    if (!G.outName) err.push_back("No output (-output) supplied.\n");
  }
  if (variant_mode(G.reportType) && !G.vcfName) err.push_back("No variant call input (-vcf) supplied; mandatory for -filter or -polish.\n");
  if (G.reportType != OP_FILTER && G.reportType != OP_SPECTRUM && G.peak == 0 && !G.peakAuto) err.push_back("No haploid peak (-peak) supplied.\n");
  if (G.reportType == OP_COMPL && !G.seqName && !G.seqDBname)
    err.push_back("No sequence meryl database (-seqmers) nor sequence (-sequence) supplied.\n");
  if (G.reportType == OP_NONE) err.push_back("No report type (-filter, -polish, -hist, -dump, -completeness) supplied.\n");
  if (!G.readDBname && G.readsNames.empty()) err.push_back("No read meryl database (-readmers) supplied.\n");
}
