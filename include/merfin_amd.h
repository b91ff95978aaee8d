/*
 * merfin_amd.h -- C ABI of the MI355X-native k-mer multiplicity evaluator.
 *
 * This is the drop-in boundary for merfin's evaluation hot path (reference:
 * arangrhie/merfin, paths below relative to /root/reference).  merfin has no
 * plugin/FFI interface; the seams that exist in its source are
 *   (1) the sweatShop callback triple  load / process / output
 *       (src/merfin/merfin.C:30-31,59-65, wired at :377,383,389),
 *   (2) the lookup object  merylExactLookup::{estimateMemoryUsage,load,value}
 *       (src/merfin/merfin-globals.C:135-159,107-108),
 *   (3) the K* parameter fields of merfinGlobal
 *       (src/merfin/merfin-globals.H:172,222-227,239).
 * Each entry point below names the seam it replaces.  Plain pointers and
 * sizes only: no C++/torch types cross this boundary.  INTEGRATION.md shows
 * the binding a merfin maintainer would add on the reference side.
 *
 * Conventions
 *   - every function returning int returns 0 on success or a negative MFX_E_*
 *     code; mfx_last_error() then returns a thread-local description.  The
 *     library never calls exit() (the reference does: merfin-globals.C:31,152).
 *   - objects are bound to the HIP device they were created on; calls may come
 *     from any host thread.  An mfx_eval is used by one thread at a time.  An
 *     mfx_seq and an mfx_index that are only READ (evaluations, lookups, dumps,
 *     variant runs) may be shared by several evaluators driven from several
 *     threads -- the slots of one device (`merfin -devices 0,0,0,0`): what a
 *     sequence makes on first use is made under a lock, and no result depends
 *     on what other threads have queued on the device.  Calls that CHANGE an
 *     object (uploads into a sequence, adds / loads into an index) need it to
 *     themselves.  `stream` arguments are hipStream_t passed as void* (NULL =
 *     the device's default stream).
 *   - k-mers are 2k-bit integers, A=0 C=1 T=2 G=3, first base most significant
 *     (meryl's kmerTiny encoding), 1 <= k <= 64 as in the reference (its kmer type holds
 *     2k <= 128 bits).  For k <= 31 a k-mer is ONE uint64_t in every array of this ABI; for
 *     32 <= k <= 64 it is TWO consecutive uint64_t words {low 64 bits, high bits}, so a
 *     `const uint64_t *kmers` argument then points to 2*n words.  The k <= 31 path is the tuned
 *     one (BASELINE's configurations use k = 21 and 31); 32 <= k <= 64 runs the plain per-lane
 *     kernels of csrc/mfx_wide.hip and does not support a sharded index.
 */
#ifndef MERFIN_AMD_H
#define MERFIN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MFX_OK            0
#define MFX_E_INVAL      -1   /* bad argument                                  */
#define MFX_E_NOMEM      -2   /* host or device allocation failed              */
#define MFX_E_HIP        -3   /* a HIP runtime call failed                     */
#define MFX_E_FULL       -4   /* index capacity exceeded                       */
#define MFX_E_OVERFLOW   -5   /* more DISTINCT far K* bins than an evaluator holds */
#define MFX_E_IO         -6   /* file could not be read / parsed               */
#define MFX_E_FORMAT     -7   /* file magic / version / layout not recognised  */
#define MFX_E_NODEVICE   -8   /* no usable HIP device                          */
#define MFX_E_NONCANON   -9   /* a sequence-only index met a non-canonical k-mer database */

const char *mfx_last_error(void);
int         mfx_last_error_code(void);   /* code of the last failing call on this thread */
const char *mfx_version(void);
int         mfx_device_count(void);
/* Optional (no reference counterpart): bring the device's context, this library's code object and the pinned-memory path up
 * now -- what the first upload would otherwise pay (~0.07 s) -- e.g. on a helper thread while the caller reads its FASTA. */
int         mfx_device_warm(int device);
/* free / total device memory in bytes (hipMemGetInfo): what a caller sizes its choice of index by (`merfin` takes the path-only index of the
 * variant modes when the full tables would not fit) */
int         mfx_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes);

/* ------------------------------------------------------------------------ */
/* Index: replaces the two merylExactLookup objects readLookup / asmLookup  */
/* (merfin-globals.H:217,220).  One device-resident table holds BOTH counts */
/* of every k-mer, so one probe serves merfinGlobal::getK(kmer,kmer,...)    */
/* (merfin-globals.C:101-110), which does four.                             */
/* ------------------------------------------------------------------------ */
typedef struct mfx_index mfx_index;

/* merylExactLookup() + estimateMemoryUsage (merfin-globals.C:134-153):
 * capacity_kmers = upper bound on distinct k-mers over both sets.  max_gb is
 * the -memory cap in GB (0 = none): creation fails with MFX_E_NOMEM when the
 * table would not fit, mirroring "Not enough memory to load databases".
 * mfx_index_estimate_gb is the SMALLEST table made for that capacity (load factor 0.7, what the cap is checked
 * against); when HBM is plentiful the table is made emptier -- down to load factor 0.45, within 0.75 of the free
 * HBM and within max_gb -- because emptier lines mean fewer second probes (MFX_LOAD_FACTOR fixes the factor). */
mfx_index *mfx_index_create(int k, uint64_t capacity_kmers, double max_gb, int device);
void       mfx_index_free(mfx_index *ix);
double     mfx_index_estimate_gb(int k, uint64_t capacity_kmers);

/* merylExactLookup::load(reader, maxMem, 0, minV, maxV), merfin-globals.C:156
 * (read DB: values outside [minV,maxV] are dropped at load, merfin.C:199-200)
 * and :159 (asm DB: unfiltered).  kmers/values: n pairs, any order; on_device
 * != 0 means the arrays already live on this index's device. */
int mfx_index_add_read(mfx_index *ix, const uint64_t *kmers, const uint32_t *values, uint64_t n,
                       uint64_t minV, uint64_t maxV, int on_device);
int mfx_index_add_asm(mfx_index *ix, const uint64_t *kmers, const uint32_t *values, uint64_t n,
                      int on_device);

/* merylFileReader(path) (merfin-globals.C:118-119,139): open a k-mer database
 * and learn k ("Make readDB first so we know the k size") and its size.
 * Accepted forms: a meryl database directory (decoder UNVALIDATED, see
 * csrc/mfx_db.cpp), `meryl print` text (<kmer>\t<count>, optionally .gz/.bz2/.xz)
 * and this library's flat binary (mfx_db_write_flat). */
#define MFX_DB_MERYL 1
#define MFX_DB_TEXT  2
#define MFX_DB_FLAT  3
typedef struct {
  int      k;
  int      format;         /* MFX_DB_*                                        */
  uint64_t n_kmers;        /* distinct k-mers stored                          */
  int      placed;         /* flat form: the records are sorted by their PLACE in the compact table (mfx_db_convert_placed) */
} mfx_db_info;
int mfx_db_probe(const char *path, mfx_db_info *out);
/* merylExactLookup::load from disk: side 0 = read DB (-min/-max apply,
 * merfin-globals.C:156), side 1 = assembly DB (:159). */
int mfx_index_load_db(mfx_index *ix, const char *path, int side, uint64_t minV, uint64_t maxV);
/* the same into several tables with ONE pass over the database: the shards of one process (mfx_index_set_shard), each
 * keeping the k-mers it owns -- the chunk is staged once and sent to every table's device */
int mfx_index_load_db_multi(mfx_index *const *ixs, uint32_t nix, const char *path, int side, uint64_t minV, uint64_t maxV);
/* this library's flat binary form of a database (interchange; no reference counterpart).  Strictly ascending k-mers
 * (the order `meryl print` lists them in, k <= 31) are written as delta-coded blocks -- 2.6 bytes per k-mer of a 30x read
 * set, decoded by the kernel that inserts them; any other order as 8-byte packed records (k <= 21) or plain arrays.
 * All forms load into the same tables (csrc/mfx_db.cpp holds the layouts). */
int mfx_db_write_flat(const char *path, int k, const uint64_t *kmers, const uint32_t *values, uint64_t n);
/* any accepted database (meryl directory, `meryl print` text, flat) -> the flat form, sorted (k <= 31), on the host: no
 * device is touched.  One pass makes every later load of the database a matter of its bytes over PCIe (a 30x human read
 * set: a minute of text parsing -> half a second).  CLI: merfin -convert <db> -output <file>.  n_kmers may be null. */
int mfx_db_convert(const char *in_path, const char *out_path, uint64_t *n_kmers);
/* ... -> the PLACED flat form (13 <= k <= 31, canonical databases): the records are not the k-mers but the numbers P of
 * csrc/mfx_place.h -- one to one with the canonical k-mers, and ascending P means ascending LINE of the sequence-only index's compact
 * table, whatever its size -- sorted and delta-coded (~3 bits more per record than the k-mer-sorted form).  What it buys: the kernel
 * that applies the database to the table (load_Kmers, merfin-globals.C:155-159, as a run pays it) walks the table line after line,
 * every line read and written once, instead of reading one random line per record.  Such a file loads into ANY table (the k-mers are
 * recovered from P on the device; only the compact table under its default placement takes the shortcut).  CLI: merfin -convert <db>
 * -placed -output <file>.  mfx_db_write_flat_placed writes one from ascending P and counts (mfx_db_place_keys gives P of k-mers: host
 * arrays, or device arrays on `device` for a tool that sorts on the GPU); both for k <= 30 -- the P of a 31-mer takes 65 bits, its file holds
 * P >> 1 with the strand bit in the record's count field and is made by mfx_db_convert_placed alone. */
int mfx_db_convert_placed(const char *in_path, const char *out_path, uint64_t *n_kmers);
int mfx_db_write_flat_placed(const char *path, int k, const uint64_t *pkeys, const uint32_t *values, uint64_t n);
int mfx_db_place_keys(int k, const uint64_t *kmers, uint64_t n, uint64_t *out, int on_device, int device);

/* The built table as a device-format image on disk: later runs on the same databases skip the decode +
 * insert (no reference counterpart; merfin rebuilds its lookup tables on every start, merfin.C:361). */
int        mfx_index_save(const mfx_index *ix, const char *path);
mfx_index *mfx_index_load(const char *path, double max_gb, int device);
/* An image is only as good as the inputs it was built from: the caller stores a digest of them (database and
 * sequence files: path, size, modification time; -min/-max) with the table and compares it on the next start;
 * mfx_index_get_origin also returns the read-count filter baked into the table, so that a run with other
 * -min/-max values can refuse the image instead of silently evaluating with the stored ones. */
int        mfx_index_set_fingerprint(mfx_index *ix, uint64_t fingerprint);
int        mfx_index_get_origin(const mfx_index *ix, uint64_t *fingerprint, uint64_t *minV, uint64_t *maxV);

/* The same image in memory, for handing a built table to the other GPUs of a node (one rank decodes the
 * k-mer databases and builds, the table then travels over xGMI -- an RCCL broadcast -- instead of every rank
 * decoding and building its own; merfin_amd/distributed.py::broadcast_index).
 *   source rank : mfx_index_image_header(ix, hdr)  -> MFX_INDEX_HEADER_BYTES describing geometry + filter
 *   other ranks : ix = mfx_index_create_from_header(hdr, max_gb, device)   (empty table of that geometry)
 *   all ranks   : mfx_index_device_image(ix, &lines, &line_bytes, &meta, &meta_bytes); move `lines` and `meta`
 *                 from the source's device buffers into the others'; then mfx_index_commit(ix) on the receivers. */
#define MFX_INDEX_HEADER_BYTES 128
int        mfx_index_image_header(const mfx_index *ix, void *hdr);
mfx_index *mfx_index_create_from_header(const void *hdr, double max_gb, int device);
int        mfx_index_device_image(mfx_index *ix, void **d_lines, uint64_t *line_bytes, void **d_meta, uint64_t *meta_bytes);
int        mfx_index_commit(mfx_index *ix);

typedef struct mfx_seq mfx_seq;

/* SEQUENCE-ONLY index: the lookup object for the report types that only ever ask it for the k-mers of -sequence --
 * -hist and -dump (merfin-histogram.C:54-64 and merfin-dump.C:44-61 call getK with the kmerIterator's fmer/rmer and
 * nothing else).  It holds exactly the canonical k-mers CLAIMED from a sequence; every later add / load only UPDATES
 * the counts of those k-mers and drops the rest (for a 30x human read set: half of the database, the sequencing-error
 * k-mers, never gets a slot).  value() of a claimed k-mer is what the full tables answer; value() of any other k-mer
 * is 0, so -completeness (merfin-completeness.C:48-144 walks the whole read database) and the variant modes (alternative
 * paths, varMer.C:76-84) need the full index of mfx_index_create and are refused on this one.
 *   ix = mfx_index_create_for_seq(k, <upper bound of the sequence's distinct k-mers: its bases>, max_gb, device);
 *   mfx_index_count_asm(ix, seq, 0)      -- claims the k-mers AND counts them into the assembly side (no -seqmers), or
 *   mfx_index_claim_seq(ix, seq, 0)      -- claims them only; the assembly counts then come from -seqmers
 *   mfx_index_load_db / mfx_index_add_*  -- update-only from here on; a further claim is an error
 * For k <= 21 the table takes a compact layout -- 8-byte slots {key 42 bits | readV 11 | asmV 11}, 16 per 128-byte line,
 * exact counts of saturated fields in a side table -- built directly in that form; a human assembly takes 96 GB and
 * -hist runs on 0.42 table lines per k-mer (MFX_SEQ_COMPACT=0 keeps the 16-byte slots).  The databases must be canonical
 * (one slot per canonical k-mer cannot answer value(fmer) + value(rmer) of a non-canonical one): a load that meets a
 * non-canonical k-mer fails with MFX_E_NONCANON and the caller builds the full index instead. */
mfx_index *mfx_index_create_for_seq(int k, uint64_t capacity_kmers, double max_gb, int device);
/* ... with the table's load factor chosen by the caller (0: by the free memory, as above; MFX_LOAD_FACTOR overrides both).  The
 * emptiest table probes fastest, but a short-lived process pays for the memory it asks for: one started behind another waits in
 * hipMalloc while the driver clears what the earlier one freed.  The `merfin` CLI asks for 0.4 (61 GB for a human assembly), a
 * resident evaluator for the default (0.18, 135 GB): profiles/r05_e2e_lf_ab.txt. */
mfx_index *mfx_index_create_for_seq_lf(int k, uint64_t capacity_kmers, double max_gb, int device, double load_factor);
mfx_index *mfx_index_create_lf(int k, uint64_t capacity_kmers, double max_gb, int device, double load_factor);     /* the full table, likewise (the CLI: 0.7) */
double     mfx_index_estimate_gb_for_seq(int k, uint64_t capacity_kmers);
int        mfx_index_claim_seq(mfx_index *ix, const mfx_seq *seq, void *stream);
/* PART of an assembly per device (round 4; config 5's -hist / -dump without any exchange): a device that evaluates some
 * contigs claims THEIR k-mers (mfx_index_claim_seq on a sequence object of those contigs), takes their assembly counts
 * from the WHOLE assembly -- asmV += 1 per occurrence of a claimed k-mer in `seq`, nothing is claimed --
 *   mfx_index_count_claimed(ix, whole_assembly, 0)
 * and loads the read database update-only as above.  value() of its contigs' k-mers is then what the full tables of the
 * whole run answer (`meryl count` of -sequence counts every contig, merfin-globals.C:182-186), the device evaluates its
 * contigs alone, and mfx_hist_run_parts adds the devices' results. */
int        mfx_index_count_claimed(mfx_index *ix, const mfx_seq *seq, void *stream);

/* Native replacement of the `meryl count k=.. <seq> output <seq>.meryl` child
 * process (merfin-globals.C:182-186): counts the canonical k-mers of every
 * contig of `seq` into the assembly side of the index, on the GPU. */
int mfx_index_count_asm(mfx_index *ix, const mfx_seq *seq, void *stream);
/* mfx_index_count_asm(ix, seq, 0) followed by mfx_index_load_db(ix, read_db_path, 0, minV, maxV) as one call: the database's
 * bytes cross PCIe while the sequence's k-mers are still being claimed and counted (the inserts wait for that kernel on the
 * device).  Same table as the two calls.  Replaces load_Kmers + the `meryl count` of -sequence, merfin-globals.C:114-163,182-186. */
int mfx_index_build_for_hist(mfx_index *ix, const mfx_seq *seq, const char *read_db_path, uint64_t minV, uint64_t maxV);
/* The same with the database's bytes moving from the moment the process starts (what the reference pays per run, load_Kmers,
 * merfin-globals.C:114-163, 155-159): mfx_db_stage_begin opens a delta-coded flat database (`merfin -convert`), takes device memory
 * for all of its blocks and lets a thread of its own read the file into it over PCIe -- under the FASTA read, the sequence upload, the
 * table's allocation and the claim / count kernel; mfx_index_build_for_hist_staged launches that kernel and, behind it, the
 * decode + update kernel over the staged blocks as their copies complete.  Same table as mfx_index_build_for_hist.  _begin returns
 * NULL (mfx_last_error says why) for any other database form, when the blocks would take more than a fifth of the free device
 * memory, or with MFX_DB_STAGE=0: the caller then takes the unstaged call.  The stage is released with mfx_db_stage_free (also
 * before it was used). */
typedef struct mfx_db_stage mfx_db_stage;
mfx_db_stage *mfx_db_stage_begin(const char *read_db_path, int device);
int           mfx_index_build_for_hist_staged(mfx_index *ix, const mfx_seq *seq, mfx_db_stage *stage, uint64_t minV, uint64_t maxV);
/* mfx_index_load_db of a staged database (side 0: -readmers, the -min/-max filter applies; 1: -seqmers): only the decode + insert kernels are
 * left to run.  What the path-only index of the variant modes loads both of its databases with (mfx_index_claim_paths). */
int           mfx_index_load_db_staged(mfx_index *ix, mfx_db_stage *stage, int side, uint64_t minV, uint64_t maxV);
void          mfx_db_stage_free(mfx_db_stage *stage);
/* Until this call the stage reads the file with a few threads only (the host is busy reading and encoding the sequence; MFX_DB_STAGE_THREADS,
 * default 8); call it when the sequence is uploaded. */
void          mfx_db_stage_boost(mfx_db_stage *stage);

/* merylExactLookup::value(kmer), merfin-globals.C:107-108, batched: for each
 * query returns the stored read and asm counts (0 when absent).  Queries are
 * looked up as given (no canonicalisation). */
int mfx_index_value(const mfx_index *ix, const uint64_t *kmers, uint64_t n,
                    uint32_t *readV, uint32_t *asmV);

typedef struct {
  int      k;
  int      canonical;      /* 1: every stored k-mer <= its reverse complement */
  uint64_t capacity;       /* slots                                           */
  uint64_t distinct;       /* occupied slots                                  */
  uint64_t bytes;          /* device bytes held by the table                  */
  int      seq_only;       /* 1: sequence-only index (mfx_index_create_for_seq) */
  int      compact;        /* 1: 8-byte slots, 16 per line (sequence-only, k <= 21) */
  uint64_t dropped;        /* adds a sequence-only index dropped (k-mers never claimed) */
} mfx_index_info;
int mfx_index_get_info(const mfx_index *ix, mfx_index_info *out);

/* copy out every stored (kmer, readV, asmV); arrays sized >= info.distinct.
 * Order unspecified.  (Test / -completeness support.) */
int mfx_index_export(const mfx_index *ix, uint64_t *kmers, uint32_t *readV, uint32_t *asmV,
                     uint64_t *n_out);

/* One side of a full index (not sharded, k <= 31) as a k-mer database: the k-mers whose count on `side` (0: read counts, 1: assembly
 * counts) is non-zero, with those counts -- byte for byte the file mfx_db_write_flat(path, k, kmers, values, n) writes for them in
 * ascending order, i.e. what `merfin -convert` makes of a database of them (its -placed form: convert the result).  With
 * mfx_reads_begin_all this is `meryl count` of the reads: count once, run every mode from the file.  The k-mers are sorted on the
 * device, one key range of at most 2^28 entries at a time (MFX_WRITE_DB_RANGE, read per call, lowers that: docs/KNOBS.md), and
 * collected on the host: peak host memory is 12 bytes per k-mer written, as for mfx_db_convert.  Nothing else may use the index during
 * the call.  n_kmers (may be NULL): the k-mers written. */
int mfx_index_write_db(const mfx_index *ix, int side, const char *path, uint64_t *n_kmers);

/* The entries with a non-zero count on `side` per top min(2k, 12) bits of their k-mer: bins[b] for b < *nbins = 2^min(2k, 12), the rest of
 * the 4096 words zero (nbins may be NULL).  The histogram mfx_index_write_db groups its key ranges by, behind the same refusals; what a
 * count in several passes cuts its key ranges with. */
int mfx_index_key_bins(const mfx_index *ix, int side, uint64_t *bins /* [4096] */, uint32_t *nbins);

/* A database written from SEVERAL tables -- the passes of a count over ascending key ranges (mfx_reads_begin_range).  append_index is the
 * device part of mfx_index_write_db (bins, key ranges, export, sort, copy) and adds the side's k-mers behind those the writer holds; the
 * smallest of them must exceed the writer's last k-mer, otherwise MFX_E_INVAL: the append adds nothing and the writer stays usable.  An
 * append of zero k-mers is fine.  n_added (may be NULL): the k-mers this append added.  close writes the file mfx_db_write_flat makes of
 * everything appended -- nothing exists at `path` before -- and frees w whatever the result; abort frees w and writes nothing.
 * mfx_index_write_db is open + append + close.  Host memory: 12 bytes per k-mer held until close -- at rest (11.4 GB at 0.95 G k-mers; the
 * streamed kind below holds 0.004 GB there and writes the same file in a third of the time: profiles/count_stream.txt).  The k-mers are kept in two contiguous arrays, allocated to the
 * exact size; an append that adds n to h held allocates arrays of h + n and moves the h into them, so WHILE IT RUNS the old and the new
 * arrays are alive together: a transient peak of 12 x (2 h + n) bytes, i.e. up to 24 bytes per k-mer at the last of many appends.  Size
 * the host for that (a read store beside it takes its share too).  A single append -- mfx_index_write_db -- allocates once. */
typedef struct mfx_db_writer mfx_db_writer;
mfx_db_writer *mfx_db_writer_open(const char *path, int k);
int  mfx_db_writer_append_index(mfx_db_writer *w, const mfx_index *ix, int side, uint64_t *n_added);
int  mfx_db_writer_close(mfx_db_writer *w, uint64_t *n_kmers);
void mfx_db_writer_abort(mfx_db_writer *w);

/* The STREAMED kind of the writer: the same calls, the same file byte for byte, without the host arrays.  open_streamed creates the spool
 * `<path>.blocks` (MFX_E_IO if it cannot; `path` itself does not exist before close).  append_index exports and sorts a key range as above,
 * then codes its blocks of 4096 k-mers ON THE DEVICE (plan and pack kernels, csrc/mfx_sort.hip, by the block rule of csrc/mfx_delta.h that
 * the host writer uses too); the packed bytes -- 2.7 per k-mer of a 30x read set instead of 12 -- cross PCIe through two pinned bounce
 * buffers and go to the spool while the next piece is copied.  What the host keeps is the directory (16 bytes per 4096 k-mers), the escapes
 * (12 bytes per count of 2^22 - 1 or more) and the carry: the fewer than 4096 k-mers behind the last full block, uploaded in front of the next
 * key range -- ranges, appends and passes need not align with blocks, and appends may come from indexes on different devices.  An append
 * that fails adds nothing: the spool is cut back to its length, directory, escapes and carry are restored.  close codes the last partial
 * block, writes header and directory, puts the spool behind them (copy_file_range where the file system has it), then the escapes, and
 * removes the spool; abort removes the spool and writes nothing.  Device memory: as the writer above plus 4095 pairs.
 * MFX_DB_TIMING prints the split (export, sort, plan, pack, copy, spool write, close) at close.
 * append_sorted takes HOST arrays, for both kinds: strictly ascending and above the writer's last k-mer, else MFX_E_INVAL and nothing is
 * added; the streamed kind codes them on the host.  info: the k-mers appended, the blocks and bytes in the spool, the escapes held, and
 * held_bytes -- the host memory that grows with the database (streamed: directory, escapes, carry; the other kind: its arrays).  Any
 * pointer may be NULL.  mfx_index_write_db_streamed is open_streamed + append_index + close. */
mfx_db_writer *mfx_db_writer_open_streamed(const char *path, int k);
int  mfx_db_writer_append_sorted(mfx_db_writer *w, const uint64_t *kmers, const uint32_t *values, uint64_t n);
int  mfx_db_writer_info(const mfx_db_writer *w, uint64_t *kmers, uint64_t *blocks, uint64_t *escapes, uint64_t *spool_bytes, uint64_t *held_bytes);
int  mfx_index_write_db_streamed(const mfx_index *ix, int side, const char *path, uint64_t *n_kmers);

/* mfx_db_merge: sorted databases combined on the device, window by window (`meryl union-sum` and its kin; one input: a filter).  The inputs
 * are 1 to 64 files in the sorted, delta-coded flat form (what -count, -convert and mfx_db_write_flat of ascending k-mers write; k <= 31), all
 * of one k; a flat file of no k-mers is an input of none in whatever form it was written.  Refused before any device is touched, with a text that names the file (MFX_E_INVAL / MFX_E_FORMAT): a placed file; a packed or
 * plain flat file, `meryl print` text or a meryl directory (run `merfin -convert` first); inputs of different k; out_path that is an input;
 * n_in of 0 or above 64; an unknown op; minV > maxV.
 * A k-mer is written iff the operation yields it and minV <= combined count <= maxV: the filter acts after the operation.  The result is byte
 * for byte what mfx_db_write_flat writes for the resulting ascending arrays, through the streamed writer above (MFX_DB_BOUNCE applies,
 * MFX_COUNT_WRITER does not); on any failure nothing exists at out_path and no spool stays.  A result of no k-mers is a valid file.
 * The key space is cut into half-open windows [lo, hi) at first k-mers of the inputs' blocks (csrc/mfx_merge.h), so that the blocks that may
 * overlap a window hold at most MFX_MERGE_RANGE pairs (default and largest value 2^26; read per call) summed over the inputs -- one block per
 * input more where no boundary allows less.  Per window the blocks are read with pread, decoded on the device into one ascending run per
 * input (records outside the window dropped), the runs merged pairwise by merge path, equal k-mers combined, the survivors compacted in
 * order and handed to the writer's encoder.  No hash table and no sort.  Host memory: 16 bytes per 4096 k-mers and 12 per escape of every
 * input, plus one window's blocks.  A block that decodes what no writer makes (k-mers that do not ascend, an escape missing from the list, a
 * count of zero) ends the call in MFX_E_FORMAT.  MFX_DB_TIMING adds read, decode, merge and combine to the writer's split.
 * stats (may be NULL): the k-mers of all inputs, the k-mers written, the k-mers the operation yields and the filter drops, the sums clamped to
 * 2^32 - 1, and the windows that held blocks. */
#define MFX_MERGE_SUM 0        /* union, counts added (saturating at 2^32 - 1) */
#define MFX_MERGE_MAX 1        /* union, largest count */
#define MFX_MERGE_MIN 2        /* union, smallest count among the inputs that hold the k-mer */
#define MFX_MERGE_INTERSECT 3  /* k-mers held by EVERY input, smallest count */
typedef struct { int op; uint64_t minV, maxV; int device; } mfx_db_merge_opts;
typedef struct { uint64_t n_in, n_out, n_filtered, n_saturated, windows; } mfx_db_merge_stats;
int mfx_db_merge(const char *const *in_paths, uint32_t n_in, const char *out_path, const mfx_db_merge_opts *o, mfx_db_merge_stats *st /* may be NULL */);
/* Set difference (`meryl difference` and what follows it): mfx_db_merge over in_paths, without the k-mers that a file of not_paths holds,
 * whatever its count there.  A k-mer is written iff the operation over in_paths yields it, no file of not_paths holds it, and
 * minV <= combined count <= maxV; the count written is the operation's over in_paths alone.  n_not == 0 is mfx_db_merge byte for byte.
 * The same input forms, refusals and "nothing at out_path on failure"; also refused: n_in + n_not > 64, a subtracted file that is the
 * output, a subtracted file of another k.  st as for mfx_db_merge (n_in: the k-mers of in_paths; n_filtered keeps its meaning);
 * *n_subtracted (may be NULL): the k-mers the operation yields and a subtracted file holds. */
int mfx_db_merge_except(const char *const *in_paths, uint32_t n_in, const char *const *not_paths, uint32_t n_not, const char *out_path,
                        const mfx_db_merge_opts *o, mfx_db_merge_stats *st /* may be NULL */, uint64_t *n_subtracted /* may be NULL */);
/* the window plan of mfx_db_merge alone (host only; tests): input i has n[i] k-mers in ceil(n[i] / 4096) blocks whose first k-mers are
 * first[i][..], ascending.  Row w of out (3 + 2 n_in words, at most cap rows are written): lo, hi, the pairs of its blocks, then per input
 * the blocks [b0, b1).  *n_windows: the windows of the plan. */
int mfx_db_merge_plan(const uint64_t *const *first, const uint64_t *n, uint32_t n_in, int k, uint64_t R, uint64_t *out, uint64_t cap, uint64_t *n_windows);

/* mfx_db_join_*: -completeness and -spectrum of a read database and an assembly's database WITHOUT a table: the sorted join of the two
 * files, window by window, ending in a reduction (csrc/mfx_join.hip).  Device memory holds one window (MFX_MERGE_RANGE pairs, the knob and
 * the windows of mfx_db_merge above), the host 16 bytes per 4096 k-mers and 12 per escape of each input: the size of the read database does
 * not matter.  The inputs are what mfx_db_merge takes -- sorted, delta-coded flat files of one k <= 31 (an assembly's: `merfin -count` of
 * its FASTA) -- and are refused in the same way before any device is touched: a placed file, a packed or plain flat file, text, a meryl
 * directory (run `merfin -convert` first), different k, null outputs, and for the spectrum copies / max_mult outside mfx_spectrum_run's
 * bounds.  A file of no k-mers is valid on either side.  A block that decodes what no writer makes ends the call in MFX_E_FORMAT, naming
 * the file; on every failure the outputs are left as they were.
 *   completeness: total64[p] / undrcpy64[p] as mfx_completeness_pieces gives them for a full index of the two files -- the same doubles
 *     (readK is an integer: the sums are exact in any order); peak, n_prob, probK, probP as in mfx_kparams; the raw read count is used,
 *     minV / maxV do not apply (as there).
 *   spectrum: img and *n_entries as mfx_spectrum_run gives them for a full index loaded with minV / maxV on the read side: a read count
 *     outside [minV, maxV] counts as 0, a read-only k-mer that becomes (0, 0) is no entry.  MFX_SPECTRUM_AGG applies.
 * stats (may be NULL): the k-mers of the two inputs, the k-mers both hold, the windows that held blocks; seconds spent in pread + copy,
 * in the decode, in launching the join (the kernel itself only with MFX_DB_TIMING set, which waits for it per window) and in the call. */
typedef struct {
  int             device;
  uint64_t        minV, maxV;          /* spectrum: -min / -max on the read count */
  double          peak;                /* completeness: mfx_kparams */
  uint32_t        n_prob;
  const uint32_t *probK;
  const double   *probP;
  uint32_t        copies, max_mult;    /* spectrum: as mfx_spectrum_run */
} mfx_db_join_opts;
typedef struct { uint64_t n_read, n_asm, n_both, windows; double t_read, t_decode, t_join, t_total; } mfx_db_join_stats;
int mfx_db_join_completeness(const char *read_path, const char *asm_path, const mfx_db_join_opts *o, double *total64, double *undrcpy64, mfx_db_join_stats *st /* may be NULL */);
int mfx_db_join_spectrum(const char *read_path, const char *asm_path, const mfx_db_join_opts *o, uint64_t *img, uint64_t *n_entries, mfx_db_join_stats *st /* may be NULL */);
/* Host only (tests, tools/native/db_join_sanitize.cpp).  grain: the merged positions a lane and a workgroup of the join kernel take at a
 * time (csrc/mfx_join.h).  host: the kernel's walk -- tiles, lane shares, the ownership of a k-mer both runs hold -- over two strictly
 * ascending host runs: one (k-mer, read count, asm count) per distinct k-mer in the order the lanes meet them, 0 for "not in that run";
 * at most cap are stored, *n_pairs counts them all. */
void mfx_db_join_grain(uint32_t *per_lane, uint32_t *tile);
int mfx_db_join_host(const uint64_t *read_keys, const uint32_t *read_vals, uint64_t n_read, const uint64_t *asm_keys, const uint32_t *asm_vals, uint64_t n_asm,
                     uint64_t *keys, uint32_t *readV, uint32_t *asmV, uint64_t cap, uint64_t *n_pairs);

/* mfx_db_diploid: TWO haplotype assemblies against the reads in one windowed pass over three sorted flat databases, ending in reductions
 * only: no table, no sort, no intermediate file, device memory holds one window (MFX_MERGE_RANGE).  It replaces the chain mfx_db_merge
 * ([hap1, hap2]) + three mfx_db_join_completeness + one mfx_db_join_spectrum, which reads the read database four times, and adds what that
 * chain cannot give: the class of a k-mer by which assembly holds it.  The rule is csrc/mfx_diploid.h, the kernels csrc/mfx_diploid.hip: the
 * two assemblies' runs are tagged, merged and compacted into one run of (k-mer, c1, c2), against which the read run is joined by
 * mfx_join_kernel; the read run is read once.
 * For every distinct k-mer of the union: r its raw read count (0: absent), rf = r where minV <= r <= maxV and else 0, c1 / c2 its counts in
 * hap1 / hap2, cb = min(c1 + c2, 2^32 - 1) (what mfx_db_merge writes with MFX_MERGE_SUM).
 *   asm_img   the class image (spectra-asm): 4 rows of max_mult + 1 cells, column min(rf, max_mult); row 0 read-only (c1 == c2 == 0), row 1
 *             hap1-only, row 2 hap2-only, row 3 shared; a k-mer with rf == 0 and cb == 0 is no entry
 *   cn_img    (copies + 2) rows of max_mult + 1 cells and *n_entries: cell for cell what mfx_db_join_spectrum(reads, M) gives for
 *             M = mfx_db_merge([hap1, hap2], SUM); the column sums of the two images are equal
 *   stats     per X in hap1, hap2, both (cX = c1, c2, cb): distinct = the k-mers with cX > 0, total = the sum of cX, only_distinct /
 *             only_total = the same over the k-mers with r == 0 (the RAW count: minV / maxV do not apply), found = the k-mers with rf > 0
 *             and cX > 0; solid = the k-mers with rf > 0; n_read, n_hap1, n_hap2 the k-mers of the inputs, n_shared those of both
 *             assemblies, windows; seconds in pread + copy, decode, tag + merge + pair run, launching the join (the kernels' own time only
 *             with MFX_DB_TIMING set, which waits per window) and in the call.  All counters are exact.
 *   total64[64], undrcpy64[3 * 64] (computed iff both are given): merfin's completeness sums as mfx_db_join_completeness defines them, for
 *             hap1, hap2 and M -- the same doubles as three calls of it (the total does not depend on the assembly); peak, n_prob, probK,
 *             probP as there.
 * QV of X: mfx_histoQV(only_total, total) (merfin-histogram.C:22-31); k-mer completeness of X: found / solid.  Both follow Merqury's QV and
 * completeness in spirit and are UNVALIDATED against Merqury; the distinct and the total counts are both given, so that a reader can apply
 * the other convention.
 * The inputs and refusals are mfx_db_merge's (sorted delta-coded flat files of one k <= 31), all before any device is touched; also refused:
 * copies / max_mult outside mfx_spectrum_run's bounds, null outputs, exactly one of total64 / undrcpy64.  hap1 and hap2 may be the same
 * file; a file of no k-mers is valid in any role.  distinct of hap1 / hap2 is checked against n_hap1 / n_hap2, the images against their
 * entry counters (MFX_E_HIP).  On every failure the outputs are left as they were. */
typedef struct { uint64_t distinct, total, only_distinct, only_total, found; } mfx_diploid_counts;
typedef struct {
  mfx_diploid_counts hap1, hap2, both;
  uint64_t solid, n_read, n_hap1, n_hap2, n_shared, windows;
  double   t_read, t_decode, t_pair, t_join, t_total;
} mfx_db_diploid_stats;
int mfx_db_diploid(const char *read_path, const char *hap1_path, const char *hap2_path, const mfx_db_join_opts *o, uint64_t *asm_img, uint64_t *cn_img,
                   uint64_t *n_entries, mfx_db_diploid_stats *st, double *total64 /* may be NULL */, double *undrcpy64 /* [3 * 64], may be NULL */);
/* Host only (tests, tools/native/diploid_sanitize.cpp): the text the kernels run -- tag, merge, head compaction, the tiled lane walk, the
 * rule -- over three strictly ascending host runs of k-mers of length k.  One (k-mer, r, c1, c2) per distinct k-mer in the order the lanes
 * meet them: at most cap are stored, *n_kmers counts them all.  Images, counters (no times; windows 0) and piece sums as above. */
int mfx_db_diploid_host(const uint64_t *read_keys, const uint32_t *read_vals, uint64_t n_read, const uint64_t *hap1_keys, const uint32_t *hap1_vals, uint64_t n_hap1,
                        const uint64_t *hap2_keys, const uint32_t *hap2_vals, uint64_t n_hap2, int k, const mfx_db_join_opts *o, uint64_t *keys, uint32_t *readV,
                        uint32_t *c1V, uint32_t *c2V, uint64_t cap, uint64_t *n_kmers, uint64_t *asm_img, uint64_t *cn_img, uint64_t *n_entries,
                        mfx_db_diploid_stats *st, double *total64 /* may be NULL */, double *undrcpy64 /* may be NULL */);
/* Host only.  The class image as text: "Assembly<TAB>kmer_multiplicity<TAB>Count", the rows labelled read-only, hap1-only, hap2-only,
 * shared, one line per non-zero cell; .gz / .bz2 / .xz names go through the compressed writers (as mfx_spectrum_write). */
int mfx_diploid_write_asm(const uint64_t *img, uint32_t max_mult, const char *path);

/* mfx_db_trio: the two hap-mer databases of a trio from the parents' databases, and optionally the child's, in one windowed pass with no
 * intermediate file (what -phase and -bin take as -hapmers A B).  The inputs are what mfx_db_merge takes -- sorted, delta-coded flat files of
 * one k <= 31 -- and share its windows (MFX_MERGE_RANGE), its pread loop, its block decode and its pairwise merge; the record's input travels
 * through the merge in the two low bits of the key (csrc/mfx_trio.h).  With cm, cp, cc a k-mer's counts in mat, pat and child (0: absent) and
 * the cutoffs tm, tp, tc >= 1:
 *   set A (maternal):  cm >= tm and cp == 0 and (no child given or cc >= tc); the count written is min(cm, cc), cm without a child
 *   set B (paternal):  cp >= tp and cm == 0 and (no child given or cc >= tc); min(cp, cc), or cp
 * so out_a is byte for byte the file of mfx_db_merge_except([mat], [pat], X, minV = tm), mfx_db_merge([child], Y, minV = tc),
 * mfx_db_merge([X, Y], out_a, INTERSECT), and out_b the same with the parents swapped.  Both outputs go through a streamed writer each;
 * a second run gives the same bytes; on any failure neither out_a nor out_b exists and no spool stays.
 * The histogram image: 3 rows of max_mult + 1 cells (max_mult as for mfx_spectrum_run: 4 to 65536), column m < max_mult the count m, the last
 * column the counts >= max_mult.  Row 0: the k-mers with cp == 0, by cm; row 1: the k-mers with cm == 0, by cp; row 2: every child k-mer, by
 * cc (all zero without a child).  It is made on the device with mfx_spectrum.h's bins (exact integer adds).
 * A cutoff of 0 is automatic: mfx_spectrum_peak(row).valley of its row (mat: row 0, pat: row 1, child: row 2), after a first pass over the
 * inputs that makes the image.  A row without a valley ends the call in MFX_E_NODATA, the text names the database and the cutoff to give
 * instead, and nothing is written.  This rule -- parent-specific k-mers above the error valley of their own histogram, kept where the child
 * holds them above its valley -- is this library's own, in the spirit of Merqury's hapmers.sh; it is UNVALIDATED against Merqury.
 * Refused before any device is touched (MFX_E_INVAL / MFX_E_FORMAT, the text names the file): a null argument, an input form mfx_db_merge
 * refuses, inputs of different k, an output that is an input, out_a and out_b the same file, cut_child != 0 without a child, max_mult out of
 * bounds.  mat and pat may be the same file: two databases of no k-mers.  MFX_E_NOMEM names the buffers of a window and of both writers.
 * img (may be NULL): filled when the first pass ran (stats->hist_pass), else left as it was.
 * stats (may be NULL), all exact: the k-mers of each input, of both parents, of one parent alone, of one parent alone at or above its cutoff,
 * the child's at or above tc, the k-mers written to A and to B, the windows that held blocks, the cutoffs used and whether each was
 * automatic; seconds in pread + copy, decode, tag + merge, the histogram kernel, the classify kernels, the writers' appends, their close and
 * the call (the kernels' own time only with MFX_DB_TIMING set, which waits for them per window). */
typedef struct { uint32_t cut_mat, cut_pat, cut_child; /* 0: automatic */ uint32_t max_mult; int device; } mfx_db_trio_opts;
typedef struct {
  uint64_t n_mat, n_pat, n_child, n_both, n_mat_only, n_pat_only, n_mat_only_cut, n_pat_only_cut, n_child_cut, n_a, n_b, windows;
  uint32_t cut_mat, cut_pat, cut_child, auto_mat, auto_pat, auto_child, hist_pass, reserved;
  double   t_read, t_decode, t_merge, t_hist, t_classify, t_write, t_close, t_total;
} mfx_db_trio_stats;
int mfx_db_trio(const char *mat_path, const char *pat_path, const char *child_path /* may be NULL */, const char *out_a, const char *out_b, const mfx_db_trio_opts *o,
                uint64_t *img /* may be NULL */, mfx_db_trio_stats *st /* may be NULL */);
/* The image of the first pass alone: img[3 * (max_mult + 1)].  stats (may be NULL): the k-mers of the inputs, of both parents, of one alone,
 * the windows and the times; the cutoffs and what depends on them stay 0.  The same inputs and refusals; nothing is written. */
int mfx_db_trio_hist(const char *mat_path, const char *pat_path, const char *child_path /* may be NULL */, uint32_t max_mult, uint64_t *img, mfx_db_trio_stats *st, int device);
/* `meryl histogram` of one sorted flat database (k <= 31), by the same pass with the file in the child's role: row[max_mult + 1], column
 * m < max_mult the k-mers of count m, the last column those of max_mult and more; *n_kmers (may be NULL) = the sum of the row = the k-mers
 * of the file.  The input forms and refusals of mfx_db_merge. */
int mfx_db_histogram(const char *path, uint32_t max_mult, uint64_t *row, uint64_t *n_kmers, int device);
/* Host only.  "count<TAB>k-mers", one line per non-zero cell, ascending; the overflow column is written as max_mult.  .gz / .bz2 / .xz
 * names go through the compressed writers.  This is the two-column k-mer histogram GenomeScope reads (what `meryl histogram` prints);
 * the layout is written from that description and UNVALIDATED against `meryl histogram`. */
int mfx_db_histogram_write(const uint64_t *row, uint32_t max_mult, const char *path);
/* Host only (tests, tools/native/trio_sanitize.cpp): the rule of csrc/mfx_trio.h -- tag, merge, head walk, class -- over three strictly
 * ascending host runs, as the kernels run it.  has_child == 0: no child (n_child must be 0).  cut_* >= 1.  a_keys / a_vals hold n_mat,
 * b_keys / b_vals n_pat records at the most; img[3 * (max_mult + 1)]; st: the counters (no times, no windows). */
int mfx_db_trio_host(const uint64_t *mat_keys, const uint32_t *mat_vals, uint64_t n_mat, const uint64_t *pat_keys, const uint32_t *pat_vals, uint64_t n_pat,
                     const uint64_t *child_keys, const uint32_t *child_vals, uint64_t n_child, int has_child, uint32_t cut_mat, uint32_t cut_pat, uint32_t cut_child,
                     uint32_t max_mult, uint64_t *a_keys, uint32_t *a_vals, uint64_t *n_a, uint64_t *b_keys, uint32_t *b_vals, uint64_t *n_b, uint64_t *img,
                     mfx_db_trio_stats *st);

/* ------------------------------------------------------------------------ */
/* Read k-mer counting: the read counts of a run straight from its reads     */
/* (FASTA / FASTQ records), no k-mer database in between.                   */
/* ------------------------------------------------------------------------ */
/* The canonical k-mers of the reads (all k bases ACGT, either case: `meryl count` / kmerIterator) are counted on the device
 * INTO the k-mers the index holds: a held k-mer's read count grows by its occurrences, any other k-mer is dropped.  The
 * index must be one whose keys are already what the run asks: a sequence-only index (mfx_index_create_for_seq + claim /
 * count of the assembly), a path-only index (mfx_index_claim_paths), or for 32 <= k <= 64 a table whose k-mers came from
 * the assembly only.  Its read side must not have taken counts (a database load, an earlier counter), and takes none from any
 * other source afterwards.  Its assembly side may come before or after for k <= 31 (updates of claimed k-mers); for 32 <= k <= 64
 * every add claims, so it must come BEFORE begin.  Counts are exact up to 2^32 - 1 (compact layout: a field reaching 2047 moves to
 * the side table as a database load does it).  After begin the index takes no more claims (MFX_E_INVAL).
 *   r = mfx_reads_begin(ix, 0);
 *   for each batch of records:  mfx_reads_add(r, bases, lens, n);   -- returns once the caller's buffers may be reused
 *   mfx_reads_end(r, &stats);                                        -- waits, checks the table (MFX_E_FULL), frees r
 * batch_bases: bases per device batch (0: 64 Mi); a read longer than the room left in a batch is split with a k-1 overlap. */
typedef struct mfx_reads mfx_reads;
typedef struct mfx_reads_stats {
  uint64_t reads, bases;     /* records and bases passed in                                   */
  uint64_t kmers;            /* valid k-mers of those reads (kmerIterator rules)              */
  uint64_t counted;          /* of those: k-mers the index answers for, added to their count  */
  uint64_t dropped;          /* the rest: not claimed (error k-mers, other haplotypes, ...)    */
  uint64_t saturated;        /* k-mers whose read count ended in the side table (a saturated compact field, or a
                                quotient-form k-mer kept there beyond its candidate lines)                          */
  double   seconds_kernel, seconds_copy;
} mfx_reads_stats;
mfx_reads *mfx_reads_begin(mfx_index *ix, uint64_t batch_bases);
/* -min / -max of the run (merfin.C:199-200): applied when the counts are looked up, as for a database; default 0, 2^64 - 1 */
int        mfx_reads_set_filter(mfx_reads *r, uint64_t minV, uint64_t maxV);
int        mfx_reads_add(mfx_reads *r, const char *const *bases, const uint64_t *lens, uint64_t n);
/* out may be NULL; r is freed whatever the result */
int        mfx_reads_end(mfx_reads *r, mfx_reads_stats *out);

/* The CLAIMING counter -- `meryl count` of the reads: every canonical k-mer of the reads is claimed if the index does not hold it, and its
 * read count grows by its occurrences.  Nothing is dropped: stats.dropped == 0 and counted == kmers.  The same object as mfx_reads_begin
 * gives, used with the same mfx_reads_add / mfx_reads_set_filter / mfx_reads_end.  The index: a full one (mfx_index_create*), 1 <= k <= 31,
 * not sharded, its read side untouched; its assembly side may be filled before or after (those adds claim as always; the index is not
 * frozen).  Refused with MFX_E_INVAL: a sequence-only or path-only index, k > 31, a sharded index, a read side that already took counts.
 * The TABLE GROWS, because nobody knows the reads' distinct k-mers beforehand; create the index small.  No launch may overfill the table:
 * a batch of B positions is enqueued only while  distinct + pending + B <= 0.7 x slots  (distinct: the table's count as last read;
 * pending: the positions enqueued since, each of which may claim a k-mer).  Otherwise the batches in flight are waited for and the count
 * is read again; if the bound still fails, every entry moves into a table of the smallest power-of-two multiple of the lines (at least
 * twice) with  distinct + B <= 0.35 x slots, and the old table is freed.  mfx_index_get_info shows the new capacity and bytes.  Both tables
 * are alive while the entries move: that sum honours the index's max_gb, the new table the free device memory.  A table that cannot grow
 * fails the mfx_reads_add (or _end) that needed it with MFX_E_NOMEM, naming both sizes; the counter is then failed, mfx_reads_end reports
 * MFX_E_NOMEM too.  Nothing was launched for the batch that needed the larger table, and the batches before it are complete: the table is
 * intact and holds their counts.  The index may still be READ -- mfx_index_get_info, mfx_index_key_bins, mfx_index_export -- and freed; it
 * takes no other counter.  A claiming counter does not end in MFX_E_FULL.
 * As for every call that changes an index: NO evaluator, replica or image of the index may exist while a claiming counter is open -- they
 * hold the table's address and geometry, and a growth replaces both. */
mfx_reads *mfx_reads_begin_all(mfx_index *ix, uint64_t batch_bases);
/* The RANGED claiming counter: as mfx_reads_begin_all, for the canonical k-mers with key_lo <= kmer < key_hi only (a k-mer as the number its
 * 2k bits are, A C G T = 0 1 2 3).  One pass of a count whose table does not fit the device: ascending ranges give ascending tables, which
 * mfx_db_writer_append_index joins into the database of one pass, byte for byte.  The conditions and refusals of mfx_reads_begin_all, and
 * MFX_E_INVAL for key_lo > key_hi and for key_hi > 4^k; key_lo == key_hi counts nothing; [0, 4^k) is mfx_reads_begin_all.
 * Statistics: `kmers` is every valid k-mer of the reads, `counted` the occurrences in the range, `dropped` 0 -- the k-mers left to other
 * passes are kmers - counted.  The growth bound counts every position of a batch as a possible claim, in range or not: pessimistic for a
 * narrow range, by one batch. */
mfx_reads *mfx_reads_begin_range(mfx_index *ix, uint64_t batch_bases, uint64_t key_lo, uint64_t key_hi);

/* The read store: the batches of a read set as the counters send them to the device (2-bit codes and validity bits, 3 bits per base), kept
 * on the host, so that the second and later passes of a count parse and decompress nothing.  It needs no device.
 *   create: k and batch_bases as for a counter (0: 64 Mi); max_bytes: the planes the store may hold (0: no limit).
 *   add: records as for mfx_reads_add (the same batching code).  MFX_OK, or 1: full -- the store is incomplete from now on and every
 *        later add returns 1; or an error (< 0).
 *   info: batches held (the one being filled included), their bytes, the records and bases passed in, complete or not (any may be NULL).
 *   mfx_reads_replay: the store's batches [first_batch, first_batch + n_batches) go through counter r -- update-only, claiming or ranged --
 *        as its own batches do (its stages, its growth bound); the records and bases those batches brought are added to r's statistics,
 *        so replaying every batch once gives the statistics of mfx_reads_add of the same records.  Refused with MFX_E_INVAL: an incomplete
 *        store, a store of another k, a counter whose batch is smaller than the store's.  Records r holds from mfx_reads_add go first.
 * A store is not changed by a replay; do not add to it from another thread meanwhile. */
typedef struct mfx_reads_store mfx_reads_store;
mfx_reads_store *mfx_reads_store_create(int k, uint64_t batch_bases, uint64_t max_bytes);
int  mfx_reads_store_add(mfx_reads_store *s, const char *const *bases, const uint64_t *lens, uint64_t n);
int  mfx_reads_store_info(const mfx_reads_store *s, uint64_t *batches, uint64_t *bytes, uint64_t *reads, uint64_t *n_bases, int *complete);
int  mfx_reads_replay(mfx_reads *r, const mfx_reads_store *s, uint64_t first_batch, uint64_t n_batches);
void mfx_reads_store_free(mfx_reads_store *s);
/* what claiming counters did to the index's table so far: growths, their wall time, of that the kernels that moved the entries, and the
 * bytes those read and wrote (any pointer may be NULL) */
int        mfx_index_growths(const mfx_index *ix, uint64_t *n, double *seconds, double *rehash_seconds, uint64_t *rehash_bytes);

/* ------------------------------------------------------------------------ */
/* Sequences: replaces the loader callback loadSequence (merfin.C:30-53) +  */
/* merfinInput::{seq,kiter} (merfin-globals.H:64-65).  All contigs are      */
/* packed into one HBM buffer once; k-mer extraction happens on the device. */
/* ------------------------------------------------------------------------ */
mfx_seq *mfx_seq_upload(int device, const char *const *bases, const uint64_t *lens, uint32_t ncontigs);
/* contigs already resident on the device, each at d_bases[i] */
mfx_seq *mfx_seq_from_device(int device, const void *const *d_bases, const uint64_t *lens, uint32_t ncontigs,
                             void *stream);
void     mfx_seq_free(mfx_seq *s);
uint32_t mfx_seq_num_contigs(const mfx_seq *s);
uint64_t mfx_seq_num_bases(const mfx_seq *s);
/* work units (contig-aligned position tiles) -- the sharding granule for
 * multi-GPU runs: rank r of N evaluates tiles [T*r/N, T*(r+1)/N). */
uint64_t mfx_seq_num_tiles(const mfx_seq *s);
/* 1: the evaluations of this sequence read its packed planes (2-bit codes + validity bits, 0.375 B per base) -- a packed upload,
 * mfx_seq_pack, a replica, and every resident sequence the library made its own copy of (mfx_seq_from_device, the one-byte-per-base
 * mfx_seq_upload): the planes are made once, where the copy is made, unless MFX_SEQ_PACK=0 or the device has no room for them;
 * 0: its launches encode their tiles from one byte per base */
int      mfx_seq_is_packed(const mfx_seq *s);

/* ------------------------------------------------------------------------ */
/* Evaluator: the K* parameters of merfinGlobal (merfin-globals.H:222-239)  */
/* bound to an index.                                                       */
/* ------------------------------------------------------------------------ */
typedef struct {
  double          peak;      /* -peak (merfin.C:89-90)                         */
  uint32_t        n_prob;    /* rows of the -prob table, 0 = none              */
  const uint32_t *probK;     /* copyKmerK (merfin-globals.H:226)               */
  const double   *probP;     /* copyKmerP (merfin-globals.H:227)               */
} mfx_kparams;

typedef struct mfx_eval mfx_eval;

/* nbins: dense K* bins kept per side on the device (0 = default 65536); bins
 * beyond are aggregated in a table of far bins (mfx_hist_take_overflow), so
 * results do not depend on it. */
mfx_eval *mfx_eval_create(const mfx_index *ix, const mfx_kparams *kp, uint32_t nbins);
void      mfx_eval_free(mfx_eval *ev);
uint32_t  mfx_eval_nbins(const mfx_eval *ev);
/* Diagnostic (no reference counterpart): random 128-byte lines per second this device's HBM delivers to independent
 * 16-byte loads over a table of table_bytes (allocated and released by the call): the roof of the index probe on this
 * box; bench.py reports the -hist kernel's line rate against it (roofline.gather_ceiling). */
int       mfx_diag_gather_rate(int device, uint64_t table_bytes, double *lines_per_s);
/* Test hook (no reference counterpart): -hist launches of this evaluator run the DEBUG instance of the kernel where one
 * exists (compact layout, k = 21) and count how its probe's queries ended: out8[0] not in the first mini-bucket (first
 * cooperative pass), [1] home line full (second cooperative pass), [2] saturated count (side table), [3] per-lane
 * whole-line scans.  mfx_eval_debug_counters reads and clears them.  Never the measured configuration. */
int       mfx_eval_debug_enable(mfx_eval *ev, int on);
int       mfx_eval_debug_counters(mfx_eval *ev, uint64_t *out8);
/* Test hooks of the -hist worklist (no reference counterpart; csrc/mfx_debug.cpp).  Over a compact, canonical table the -hist
 * kernel lists the rare endings of its probe in one segment per block and a second kernel ends them; the result must not depend
 * on what was listed.  mfx_eval_debug_worklist: how every later -hist launch of this evaluator (all launch forms) gets its list --
 * mode 0 none, 1 the default sizing, 2 a segment holds at most min(default, segcap) entries (segcap >= 1; the allocation is the
 * default's).  mfx_eval_debug_worklist_read: the list of the last launch of launch slot 0 / 1 (a plain launch uses slot 0, a
 * streamed run's chunks alternate), after synchronising the device: *segs segments of at most *segcap entries (0, 0: that launch
 * had no list), counts[*segs] entries per segment, *n_entries their sum, and the entries themselves, segment after segment, as
 * 16-byte records { u64 canonical k-mer; u32 aux; u32 slot | mode << 29 | dbl << 31 } with slot = (tile of the launch) * 4 +
 * wave.  counts / entries may be NULL (sizes first); *_cap: what the caller's buffers hold (words / records).  Everything is
 * checked against the list's allocation before it is copied. */
int       mfx_eval_debug_worklist(mfx_eval *ev, int mode, uint32_t segcap);
int       mfx_eval_debug_worklist_read(mfx_eval *ev, int slot, uint32_t *segs, uint32_t *segcap, uint64_t *counts, uint64_t counts_cap,
                                       void *entries, uint64_t entries_cap, uint64_t *n_entries);

/* Test hooks of the variant modes (no reference counterpart; csrc/mfx_debug.cpp): the per-path values of the traverse and score
 * kernels, which a run only shows after bestFilter / bestVariant / ... have reduced them.  The cluster tables are raw arrays of
 * csrc/mfx_traverse.h's structs, little endian, no padding beyond the named fields:
 *   cluster 56 B  { u64 win_off; u32 win_len, nv, var0, path_cap; u64 text0, path0, row0; u32 text_cap, pad; }
 *   variant 16 B  { u32 off, reflen, na, al0; }          allele 16 B  { u64 off; u32 len, pad; }
 * A cluster's paths go to text[text0 ...] (each followed by '\n'; room text_cap), path slots path0 ... (room path_cap) and rows
 * row0 + path * nv + variant.  status: 0 ok, 1 a replacement past the end of its string (std::string::replace throws there),
 * 2 a limit or the reserved room exceeded.  Every offset is checked against its array first (MFX_E_INVAL).
 *
 * mfx_debug_traverse_host: the shared traverse (the code the device runs one wave per cluster) in its one-thread form, on the
 * host; no device is opened.  text[text_end] is the caller's (filled with '\n' by the caller where it wants to see what stays
 * untouched); the slots a cluster does not use are closed as the device closes them (length 0, cfirst = the slot itself). */
int mfx_debug_traverse_host(const void *clusters, uint64_t ncl, const void *variants, uint64_t nvar, const void *alleles, uint64_t nal,
                            const char *win_text, uint64_t win_bytes, const char *al_text, uint64_t al_bytes, uint64_t text_end,
                            uint64_t path_cap, uint64_t row_cap, uint32_t *np, uint32_t *status, char *text, uint64_t *p_off,
                            uint32_t *p_len, uint32_t *p_nv, uint64_t *p_voff, uint64_t *p_cfirst, int32_t *gt, uint32_t *vidx,
                            uint32_t *vlen);
/* varMer::score of host-enumerated paths on the device (what the variant modes run for clusters beyond the device traverse's
 * limits): path p is text[off[p] .. + plen[p]), its nv[p] rows start at voff[p] in gt / vidx / vlen [nvals], cfirst[p] is the
 * first path of its cluster.  Out: numM[npaths] and, need_dk, totdk[npaths]. */
int mfx_debug_score_paths(mfx_eval *ev, const char *text, uint64_t len, uint64_t npaths, uint64_t nvals, const uint64_t *off,
                          const uint32_t *plen, const uint32_t *nv, const uint64_t *voff, const uint64_t *cfirst, const int32_t *gt,
                          const uint32_t *vidx, const uint32_t *vlen, int need_dk, uint32_t *numM, double *totdk);
/* the same with clusters enumerated ON THE DEVICE behind a host part (text / path table as above, may be empty): the clusters'
 * text0 is absolute in the batch text and lies in [len, text_end]; path0 / row0 count from 0 behind the host's paths / rows, and
 * every one of the path_cap slots belongs to exactly one cluster.  Out: numM / totdk [npaths + path_cap] (device part behind the
 * host's), np / status [ncl], and what a run leaves on the device: text_out[text_end] (the whole batch text, '\n' where nothing
 * was written), the device part's path table p_off / p_len / p_nv / p_voff / p_cfirst [path_cap] (p_voff, p_cfirst absolute:
 * + nvals / + npaths) and rows gt_out / vidx_out / vlen_out [row_cap]. */
int mfx_debug_score_paths_trv(mfx_eval *ev, const char *text, uint64_t len, uint64_t npaths, uint64_t nvals, const uint64_t *off,
                              const uint32_t *plen, const uint32_t *nv, const uint64_t *voff, const uint64_t *cfirst, const int32_t *gt,
                              const uint32_t *vidx, const uint32_t *vlen, const void *clusters, uint64_t ncl, const void *variants,
                              uint64_t nvar, const void *alleles, uint64_t nal, const char *win_text, uint64_t win_bytes,
                              const char *al_text, uint64_t al_bytes, uint64_t text_end, uint64_t path_cap, uint64_t row_cap, int need_dk,
                              uint32_t *numM, double *totdk, uint32_t *np, uint32_t *status, char *text_out, uint64_t *p_off,
                              uint32_t *p_len, uint32_t *p_nv, uint64_t *p_voff, uint64_t *p_cfirst, int32_t *gt_out, uint32_t *vidx_out,
                              uint32_t *vlen_out);

/* merfinGlobal::getK(kmvalu,kmvalu,...) + getKmetric on the host, bit-exact
 * with the device code (merfin-globals.C:66-98, merfin-globals.H:248-261). */
void mfx_getK(const mfx_kparams *kp, uint32_t readV, uint32_t asmV,
              double *readK, double *asmK, double *prob);
double mfx_getKmetric(double readK, double asmK);
/* histoQV (merfin-histogram.C:22-31) */
double mfx_histoQV(double kval, double ktot, int k);

/* ------------------------------------------------------------------------ */
/* -hist: replaces processHistogram + outputHistogram                       */
/* (merfin-histogram.C:35-92, 96-136).                                      */
/* ------------------------------------------------------------------------ */
typedef struct {
  uint64_t  kasm;              /* histKasm     (merfin-globals.H:184)          */
  uint64_t  kmissing;          /* histKmissing (:185)                          */
  double    koverCpy;          /* histKoverCpy (:186)                          */
  uint32_t  undrMax, overMax;  /* histUndrMax / histOverMax (:188,191)         */
  uint64_t *undr, *over;       /* histUndr / histOver                          */
  uint32_t  ncontigs;
  uint64_t *contig_kasm;       /* per-contig s->kasm     (merfin-histogram.C:58)  */
  uint64_t *contig_kmissing;   /* per-contig s->kmissing (merfin-histogram.C:67)  */
} mfx_hist_result;

/* whole assembly on this object's device; result arrays are allocated by the
 * library, release with mfx_hist_result_free. */
int  mfx_hist_run(mfx_eval *ev, const mfx_seq *seq, mfx_hist_result *out);
void mfx_hist_result_free(mfx_hist_result *r);

/* The same with the upload inside: SURVEY 8(d)'s evaluate phase, "first tile H2D start -> final reduced histogram
 * on host".  `seq` = mfx_seq_create(device, lens, n) (layout + device buffers, no bases yet); bases[i] = host
 * buffer of contig i (pinned or pageable, ASCII).  The assembly crosses PCIe PACKED: host threads encode it into
 * 2-bit codes + one validity bit per base (0.375 B/base; mfx_pack_bases below -- the kmerIterator encoding of
 * merfin.C:45 moved in front of the bus) chunk by chunk, while the previous chunk is on the copy stream and the one
 * before is evaluated; the kernel reads its tiles from the packed planes.  Chunks grow from 8 MB to 128 MB of bases;
 * consecutive launches alternate between two streams so that one's first blocks fill the CUs the other's last blocks
 * leave.  3 Gb: 36.5 ms against 33.4 ms for the resident run (56 ms with one byte per base on the bus).  The result
 * is bit-identical to mfx_seq_upload + mfx_hist_run (koverCpy included: the per-tile values are summed once, at the
 * end).  Afterwards `seq` holds the whole assembly and can be used like an uploaded one (the kernels that read one
 * byte per base unpack the planes on first use).  k > 31 and MFX_STREAM_ASCII=1: one byte per base, 64 MB chunks,
 * pinned buffers DMA'd in place, pageable ones staged through pinned memory. */
void    *mfx_host_alloc(size_t bytes);
void     mfx_host_free(void *p);
mfx_seq *mfx_seq_create(int device, const uint64_t *lens, uint32_t ncontigs);
int      mfx_hist_run_streamed(mfx_eval *ev, mfx_seq *seq, const char *const *bases, mfx_hist_result *out);
/* The same over N devices driven by one process (the reference is one binary driving its workers, merfin.C:366-414; SURVEY 8(d) asks
 * for the evaluate phase "at 1/2/4/8 GPUs"): device d receives only the packed planes of ITS share of the tiles -- the contiguous
 * stretch [T d / N, T (d + 1) / N), cut at multiples of 1024 tiles, plus the k - 1 bases of halo behind it -- over its own copy
 * stream from its own encoder threads, and evaluates the chunks as they land; the images are added on the host in slot order.  The
 * result is bit-identical to mfx_hist_run_streamed / mfx_hist_run on one device, koverCpy included (the first-level sums of the
 * (tile, wave) values are the single launch's own, and the host adds them in the device's order).  Every slot needs its own
 * evaluator and its own sequence object (mfx_seq_create on the slot's device; evaluators on replicas of one index); afterwards a
 * slot's sequence object holds its part only and refuses whole-sequence calls (MFX_E_INVAL) until something is uploaded whole. */
int      mfx_hist_run_streamed_multi(mfx_eval *const *evs, mfx_seq *const *seqs, uint32_t ndev, const char *const *bases, mfx_hist_result *out);
/* One rank's share of it for the one-process-per-GPU launcher (bench.py, merfin_amd.mgpu): the tiles [tile_begin, tile_end) are
 * encoded, uploaded and evaluated, counts and koverCpy are ADDED to the caller's device image (MFX_HIST_WORDS(nbins, ncontigs) words
 * and one double, cleared by the caller), which the launcher then all-reduces (mfx_hist_allreduce).  Returns when the device is
 * done.  mfx_hist_stream_share: the bounds rank r of n takes (the same cut as the one-process run). */
int      mfx_hist_run_streamed_range(mfx_eval *ev, mfx_seq *seq, const char *const *bases, uint64_t tile_begin, uint64_t tile_end,
                                     uint64_t *d_counts, double *d_kover);
int      mfx_hist_stream_share(uint64_t ntiles, uint32_t rank, uint32_t nranks, uint64_t *tile_begin, uint64_t *tile_end);
/* How the bases of a streamed run cross the link is chosen per call (mfx_hist_run_streamed / _multi / _range) from two measured rates: what
 * the host threads the call has ENCODE, and what the device's LINK moves from pinned memory.  While the encoders are the faster the bases
 * cross packed (above); when they are not -- a rank of N processes has 1/N of the host's cores and a link of its own -- pinned sources cross as
 * plain bytes by DMA, no host thread touches them, and the planes are made on the device (mfx_pack_kernel); the evaluation is the same
 * launches over the same planes, the result the same bit for bit.  MFX_STREAM_TRANSPORT=pack | ascii forces either.
 * mfx_diag_stream_rates measures the two rates on demand (nothing cached): `threads` host threads encoding n bases of `src` at once, and --
 * src pinned -- up to 256 MB of it over `device`'s link; 0 for a rate that could not be measured. */
int      mfx_diag_stream_rates(int device, const char *src, uint64_t n, uint32_t threads, double *enc_gbs, double *link_gbs);
/* The host-side encoder of that transport (AVX-512 / AVX2 / scalar, chosen at run time; ~28 GB/s per core of an EPYC
 * 9575F): n bases -> ceil(n/32) words.  codes[w] holds bases 32w..32w+31, the first in the two HIGHEST bits,
 * code = (c >> 1) & 3 (A 0, C 1, T 2, G 3, either case); valid[w] holds one bit per base, the first in the highest
 * bit, set iff the base is one of ACGTacgt.  A last partial word is zero-filled. */
void     mfx_pack_bases(const uint8_t *src, uint64_t n, uint64_t *codes, uint32_t *valid);

/* Several GPUs of one node driven by ONE process -- the reference is one binary driving all its workers
 * (merfin.C:366-414).  The index is replicated (mfx_index_replicate: peer copy over xGMI, instead of N builds),
 * so is the packed assembly; slot d evaluates the block-cyclic share d of ndev of the tiles (blocks of 256 tiles)
 * on its own device and stream, all at once; the ndev counts images (~1 MB) are added on the host in slot order,
 * the overflow lists of all evaluators folded in.  Integers are exact, koverCpy is a fixed-order sum: results are
 * bit-stable and equal to the single-device ones in every integer.  Two slots may name the same device (each
 * needs its own evaluator; they may share one index and one mfx_seq). */
mfx_index *mfx_index_replicate(const mfx_index *src, int device);
mfx_seq   *mfx_seq_replicate(const mfx_seq *src, int device);
/* n replicas at once, out[i] on devices[i]: a DOUBLING TREE over xGMI -- in every round each device that holds the data
 * feeds one that does not, all copies of a round in flight together (xGMI is point to point: 7 replicas take 3 rounds with
 * 1, 2, 4 source devices instead of 7 copies through device 0's links).  The assembly travels as its packed planes
 * (0.375 B/base; mfx_seq_pack builds them on the device); a replica holds the planes and unpacks on demand.  On failure
 * nothing is left allocated. */
int        mfx_index_replicate_many(const mfx_index *src, const int *devices, uint32_t n, mfx_index **out);
int        mfx_seq_replicate_many(const mfx_seq *src, const int *devices, uint32_t n, mfx_seq **out);
int        mfx_seq_pack(mfx_seq *seq);
int        mfx_hist_run_multi(mfx_eval *const *evs, const mfx_seq *const *seqs, uint32_t ndev, mfx_hist_result *out);
/* PARTS of one assembly, one per slot: slot d evaluates ITS contigs (seqs[d]) on its own sequence-only index (their k-mers
 * claimed, assembly counts from the whole assembly by mfx_index_count_claimed, the read database update-only) -- no k-mer
 * ever leaves its device, whatever the size of the read database.  contig_ids[d][i] = number of slot d's contig i in the
 * whole assembly (ncontigs_total of them); bins and counters are added, the per-contig counters placed by those numbers,
 * koverCpy summed in slot order.  The reference's own way to spread a large run -- contigs over processes,
 * scripts/parallel1/merfin.sh:68-85 -- inside one process, with the lookup object cut to each part. */
int        mfx_hist_run_parts(mfx_eval *const *evs, const mfx_seq *const *seqs, const uint32_t *const *contig_ids, uint32_t ndev,
                              uint32_t ncontigs_total, mfx_hist_result *out);

/* One process per GPU (torchrun / mpirun style launchers): the collective of the path, on RCCL over xGMI.
 * Rank 0 makes an id (mfx_comm_unique_id), the launcher hands its MFX_COMM_ID_BYTES to every rank by any
 * out-of-band channel, every rank calls mfx_comm_create (collective).  mfx_hist_allreduce turns the ranks'
 * counts images (mfx_hist_launch / mfx_hist_launch_cyclic output) into the global one IN PLACE on every rank:
 * ncclAllReduce(sum, uint64) of the image; koverCpy = the ranks' values all-gathered and added in rank order
 * (bit-stable, whatever algorithm RCCL picks).  If the reduced image's novf word (index 2*nbins + 2) is
 * non-zero, K* bins >= nbins were seen: every rank then calls mfx_hist_allgather_overflow (collective) and folds
 * the records of all ranks with mfx_hist_result_add_overflow.  Asynchronous on `stream` except where noted. */
#define MFX_COMM_ID_BYTES 128
typedef struct mfx_comm mfx_comm;
int       mfx_comm_unique_id(void *id);
mfx_comm *mfx_comm_create(const void *id, int rank, int nranks, int device);
void      mfx_comm_free(mfx_comm *c);
int       mfx_comm_rank(const mfx_comm *c);
int       mfx_comm_size(const mfx_comm *c);
int       mfx_comm_barrier(mfx_comm *c, void *stream);      /* all ranks arrived and `stream` drained (synchronous) */
int       mfx_hist_allreduce(mfx_comm *c, uint64_t *d_counts, double *d_kover, uint32_t nbins, uint32_t ncontigs, void *stream);
/* synchronises `stream`; records[] (2 * cap words) receives the two-word records of all ranks in rank order; *n_out = records */
int       mfx_hist_allgather_overflow(mfx_comm *c, mfx_eval *ev, uint64_t *records, uint64_t cap, uint64_t *n_out, void *stream);
/* The exchange step of the sharded index (config 5: "allToAllv of the routed k-mers") for the
 * one-process-per-GPU form: group r of d_send (send_counts[r] elements of elem_bytes, groups back to back in rank order:
 * what mfx_route_tiles writes) goes to rank r; the groups arrive in source-rank order.  mfx_comm_exchange_counts tells
 * every rank what it will receive (all-gather of the count rows; synchronises `stream`), mfx_comm_alltoallv moves one
 * array (one RCCL group of point-to-point sends / receives over xGMI; asynchronous on `stream`). */
int       mfx_comm_exchange_counts(mfx_comm *c, const uint64_t *send_counts, uint64_t *recv_counts, void *stream);
int       mfx_comm_alltoallv(mfx_comm *c, const void *d_send, const uint64_t *send_counts, void *d_recv, const uint64_t *recv_counts,
                             uint32_t elem_bytes, void *stream);
/* fold n overflow records (two words each: mfx_hist_take_overflow / mfx_hist_allgather_overflow format) into a result */
int       mfx_hist_result_add_overflow(mfx_hist_result *r, const uint64_t *records, uint64_t n);

/* Device-side accumulate for sharded runs.  d_counts: uint64[MFX_HIST_WORDS]
 * caller-owned device memory, added into (zero it first), layout
 *   [0,nbins) undr | [nbins,2nbins) over | kasm | kmissing | novf |
 *   contig_kasm[ncontigs] | contig_kmissing[ncontigs]
 * d_kover: double[1], receives (+=) this launch's koverCpy.  Evaluates tiles
 * [tile_begin, tile_end).  Asynchronous on `stream`.  All-reduce d_counts and
 * d_kover over ranks to obtain the global result (the only collective). */
#define MFX_HIST_WORDS(nbins, ncontigs) (2ull * (nbins) + 3ull + 2ull * (ncontigs))
int mfx_hist_launch(mfx_eval *ev, const mfx_seq *seq, uint64_t tile_begin, uint64_t tile_end,
                    uint64_t *d_counts, double *d_kover, void *stream);
/* The same for the block-cyclic share of `rank` out of `nranks`: the tiles are cut into blocks of `block_tiles`
 * (a power of two) and rank r evaluates blocks r, r + nranks, ...  Every rank then sees every region of the assembly,
 * so a positional skew of the per-k-mer cost (repeats, k-mers that sit in overflow lines of the table) cannot make
 * one rank the straggler, which a contiguous split allows (profiles/r01_shard_timing.txt). */
int mfx_hist_launch_cyclic(mfx_eval *ev, const mfx_seq *seq, uint32_t rank, uint32_t nranks, uint32_t block_tiles,
                           uint64_t *d_counts, double *d_kover, void *stream);
/* turn an (all-reduced, host-resident) d_counts/d_kover image into a result
 * (pure host code: usable without a device, e.g. on the reducing rank) */
int mfx_hist_result_from_counts(uint32_t nbins, const uint64_t *h_counts, double kover,
                                uint32_t ncontigs, mfx_hist_result *out);
/* K* bins >= nbins seen by launches on this evaluator since the last call.  The reference's histogram arrays grow without a
 * bound (increaseArray, merfin-histogram.C:74,87); here the far bins are AGGREGATED on the device, {bin -> occurrences}, so any
 * number of k-mers may fall there (an assembly's satellite array the reads under-represent puts millions of positions into a
 * few far bins); only the number of DISTINCT far bins per evaluator is bounded (2^20; beyond: MFX_E_OVERFLOW, create the
 * evaluator with a larger nbins).  Copies up to `cap` records of TWO words each -- {bit 63 = 1 for `over` | bin index,
 * occurrences} --, sorted by the first word; *n_out = records; the evaluator's table is emptied. */
int mfx_hist_take_overflow(mfx_eval *ev, uint64_t *records, uint64_t cap, uint64_t *n_out);

/* reportHistogram (merfin-histogram.C:140-176): the histogram file text and
 * the stderr summary, byte-identical formatting.  Either path may be NULL;
 * a path ending in .gz/.bz2/.xz is piped through the matching compressor as
 * compressedFileWriter does. */
int mfx_hist_report(const mfx_hist_result *r, int k, const char *hist_path, const char *summary_path);

/* ------------------------------------------------------------------------ */
/* Sharded index (BASELINE config 5: a read DB too large for one GPU).  The  */
/* reference has no counterpart (it needs the whole DB in one host's RAM,    */
/* merfin-globals.C:148-153).  Every rank keeps the k-mers it OWNS (owner =  */
/* f(minimizer)); -hist routes each k-mer of the rank's sequence tiles to its */
/* owner, which probes, computes K* and bins; one all-reduce of the counts   */
/* image finishes.  Requires a canonical DB and odd k.                       */
/* ------------------------------------------------------------------------ */
/* call before any add/load/count: afterwards they silently skip foreign k-mers */
int mfx_index_set_shard(mfx_index *ix, uint32_t rank, uint32_t nranks);

typedef struct mfx_router mfx_router;
mfx_router *mfx_router_create(const mfx_index *ix, uint32_t nranks, uint32_t max_tiles);
void        mfx_router_free(mfx_router *r);
/* Source side: canonical k-mers of tiles [tile_begin, tile_end) grouped by owner
 * rank (sequence order kept inside a group), written to the caller's device
 * buffers d_keys_out / d_contigs_out (capacity (tile_end-tile_begin)*4096);
 * h_dest_counts[nranks] receives the group sizes.  The valid-k-mer counts
 * (kasm, per-contig kasm; merfin-histogram.C:58) are added to d_counts.
 * Synchronises `stream` once (the group sizes are needed on the host). */
int mfx_route_tiles(mfx_router *r, const mfx_seq *seq, uint64_t tile_begin, uint64_t tile_end, uint32_t nbins,
                    uint64_t *d_counts, uint64_t *d_keys_out, uint32_t *d_contigs_out, uint64_t *h_dest_counts,
                    void *stream);
/* Owner side: probe + K* + bin n received k-mers; adds bins, kmissing (global
 * and per contig) and koverCpy -- NOT kasm, which the source counted. */
int mfx_hist_keys_launch(mfx_eval *ev, const uint64_t *d_keys, const uint32_t *d_contigs, uint64_t n,
                         uint32_t ncontigs, uint64_t *d_counts, double *d_kover, void *stream);
/* The whole sharded -hist driven by ONE process: slot d = {evaluator on shard d of ndev, router on that shard,
 * the packed assembly on the shard's device}.  Rounds of route -> peer copies of the groups to their owners (xGMI)
 * -> mfx_hist_keys_launch at the owner -> counts images added on the host, overflow lists folded.  Slots may share a
 * device.  (The one-process-per-GPU form of the same loop is merfin_amd/distributed.py::sharded_hist.) */
int mfx_hist_run_sharded(mfx_eval *const *evs, mfx_router *const *routers, const mfx_seq *const *seqs, uint32_t ndev,
                         mfx_hist_result *out);

/* ------------------------------------------------------------------------ */
/* -dump: replaces processDump + outputDump (merfin-dump.C:20-68, 72-104).  */
/* ------------------------------------------------------------------------ */
/* Raw per-position values: for k-mer start positions [pos_begin,pos_end) of
 * contig `contig`, readV[i]/asmV[i] = summed read / asm counts of the k-mer
 * starting there (0,0 where no valid k-mer starts).  Host output arrays.
 * The counters are those of the range: kasm is the number of positions in
 * [pos_begin,pos_end) where a valid k-mer starts; kmissing is those of them
 * whose readK == 0 by getK (merfin-globals.C:66-98). */
int mfx_dump_values(mfx_eval *ev, const mfx_seq *seq, uint32_t contig, uint64_t pos_begin, uint64_t pos_end,
                    uint32_t *readV, uint32_t *asmV, uint64_t *kasm, uint64_t *kmissing);
/* The complete -dump of one contig appended to `path` in the reference's text
 * format "%s\t%lu\t%.2f\t%.2f\t%.2f\n" (merfin-dump.C:88-93). */
int mfx_dump_contig(mfx_eval *ev, const mfx_seq *seq, uint32_t contig, const char *name,
                    const char *path, int append, uint64_t *kasm, uint64_t *kmissing);
/* Several host threads running library calls side by side (the slots of `merfin -devices`): a thread that declares
 * itself one of `nsharers` gets 1/nsharers of the host threads in the calls it makes from then on (text formatting,
 * VCF parsing, path enumeration, staging copies) instead of all of them -- N callers each spawning a full set only
 * fight for the cores.  Thread-local; 1 = the default. */
void mfx_host_threads_share(unsigned nsharers);

/* -dump over an index SHARDED across nslots evaluators (slot d = shard d of nslots, mfx_index_set_shard; seqs[d] =
 * the same sequences resident on slot d's device; slots may share a device).  Every k-mer has one owner and the
 * other shards answer 0, so each slot looks its copy of the range up in its own shard and the value arrays are added
 * on slot 0's device (8 B per position and slot over xGMI); kmissing is counted from the sums.  Same results as
 * mfx_dump_values / mfx_dump_contig on the whole index (merfin-dump.C:44-67 sees one lookup object either way). */
int mfx_dump_values_sharded(mfx_eval *const *evs, const mfx_seq *const *seqs, uint32_t nslots, uint32_t contig,
                            uint64_t pos_begin, uint64_t pos_end, uint32_t *readV, uint32_t *asmV,
                            uint64_t *kasm, uint64_t *kmissing);
int mfx_dump_contig_sharded(mfx_eval *const *evs, const mfx_seq *const *seqs, uint32_t nslots, uint32_t contig,
                            const char *name, const char *path, int append, uint64_t *kasm, uint64_t *kmissing);

/* ------------------------------------------------------------------------ */
/* -track: K* summarised per fixed window of every contig, on the device.    */
/* The evaluation is -dump's (merfin-dump.C:44-67); what it replaces is the  */
/* post-processing of the reference README, section "Assess collapses and    */
/* duplications": -dump text -> awk -> wigToBigWig.  Per-base values never    */
/* leave the device; one record per window comes back.                       */
/* ------------------------------------------------------------------------ */
/* Window w of contig c covers the k-mer start positions [w*W, min((w+1)*W, len_c)) -- column 2 of -dump, the index of
 * mfx_dump_values.  A contig has ceil(len_c / W) windows (none when len_c == 0); the windows of contig c follow those
 * of contig c-1.  Every field is an integer sum (or a min / max): the records do not depend on the order the device
 * met the k-mers in.  Fixed layout, 72 bytes. */
typedef struct mfx_track_window {
  uint32_t n_kmers;        /* valid k-mers starting in the window (kasm, merfin-dump.C:48)                      */
  uint32_t n_missing;      /* ... of those, readK == 0 (merfin-dump.C:56)                                      */
  uint32_t n_scored;       /* ... of those, readK != 0 and K* finite: the sums, min and max are over these     */
  uint32_t n_pos;          /* scored, K* > 0 (collapsed)                                                       */
  uint32_t n_neg;          /* scored, K* < 0 (expanded)                                                        */
  uint32_t n_nonfinite;    /* readK != 0 and asmK == 0 (a foreign -seqmers: getKmetric divides by 0); in no sum */
  uint64_t sum_readK;      /* exact: readK and asmK are integer-valued for every k-mer                         */
  uint64_t sum_asmK;
  uint64_t sum_kstar_lo;   /* sum of K* as a signed 128-bit integer in units of 2^-52 (exact): low word ...     */
  int64_t  sum_kstar_hi;   /* ... and high word                                                                */
  double   min_kstar;      /* +inf when n_scored == 0                                                          */
  double   max_kstar;      /* -inf when n_scored == 0                                                          */
} mfx_track_window;
/* windows of the whole sequence set for window length `window` (0 when window == 0) */
uint64_t mfx_track_num_windows(const mfx_seq *seq, uint64_t window);
/* The records of the whole sequence set (merfin-dump.C:44-67 per k-mer, reduced per window by the kernel) into the host
 * array out[cap]; *n_out = their number, *kasm / *kmissing = the totals -hist and -dump count.  MFX_E_INVAL: window == 0,
 * cap too small, a sharded index, a sequence object that holds a part only; MFX_E_NOMEM: the records do not fit the device. */
int mfx_track_run(mfx_eval *ev, const mfx_seq *seq, uint64_t window, mfx_track_window *out, uint64_t cap, uint64_t *n_out,
                  uint64_t *kasm, uint64_t *kmissing);
/* Host only.  tsv_path: "#name start end n_kmers n_missing n_scored n_pos n_neg sum_readK sum_asmK mean_kstar min_kstar
 * max_kstar" and one tab-separated line per window with n_kmers > 0; bedgraph_path: a bedGraph track of mean K* (windows
 * with n_scored > 0) -- what the README's "Assess collapses and duplications" makes from the -dump text.  Either path may
 * be NULL; .gz / .bz2 / .xz names go through the compressed writers.  names[c]: the contig names (up to the first blank). */
int mfx_track_write(const mfx_track_window *w, uint64_t n, const mfx_seq *seq, const char *const *names, uint64_t window,
                    const char *tsv_path, const char *bedgraph_path);

/* ------------------------------------------------------------------------ */
/* -regions: maximal runs of missing, collapsed and expanded k-mers as       */
/* intervals, made on the device.  The evaluation is -dump's                 */
/* (merfin-dump.C:44-67); what it replaces is the awk over the -dump text of */
/* the reference README, "Assess collapses and duplications" (and Merqury's  */
/* meryl-lookup -bed + bedtools merge for the missing k-mers).  Per-base     */
/* values never leave the device; one record per interval comes back.        */
/* ------------------------------------------------------------------------ */
/* The class of a k-mer start position (readK, asmK = asmV, K* as -dump computes them; t = mfx_regions_opts::kstar):
 *   MISSING    a valid k-mer with readK == 0 (merfin-dump.C:56)
 *   COLLAPSED  readK != 0, asmV != 0, K* >= t   (double compare; equality is in)
 *   EXPANDED   readK != 0, asmV != 0, K* <= -t
 * A position with no valid k-mer, with |K*| < t or with a K* that is not finite (readK != 0, asmV == 0: -track's n_nonfinite)
 * is in no class.  An elementary run is a maximal stretch of consecutive positions of one contig in one class; a region
 * joins runs of one class and contig while at most `gap` positions (of any other class, or none) lie between one run's last
 * position and the next run's first -- regions of different classes may overlap, none crosses a contig's end; a region
 * of fewer than min_kmers flagged k-mers is dropped after the joining.  Records are ordered by contig, start, class.  Every
 * field is an integer sum or a max / min: the records do not depend on the order the device met the k-mers in.  56 bytes. */
enum { MFX_REGION_MISSING = 0, MFX_REGION_COLLAPSED = 1, MFX_REGION_EXPANDED = 2 };
typedef struct mfx_region {
  uint32_t contig, cls;
  uint64_t start, end;     /* k-mer start positions [start, end): first flagged .. last flagged + 1 */
  uint64_t n_kmers;        /* flagged k-mers in it (end - start minus bridged positions)            */
  uint64_t sum_readK;      /* integer-valued readK summed (0 for missing)                           */
  uint64_t sum_asmK;       /* asmV summed                                                           */
  double   ext_kstar;      /* collapsed: largest K*; expanded: smallest K*; missing: 0.0            */
} mfx_region;
typedef struct { double kstar; uint64_t gap; uint64_t min_kmers; } mfx_regions_opts;     /* -kstar (finite, > 0), -gap, -minrun */
typedef struct mfx_regions mfx_regions;                       /* the result, held by the library */
/* The records of the whole sequence set into *out (release with mfx_regions_free); *kasm / *kmissing = the totals -hist and
 * -dump count.  Two passes (csrc/mfx_regions.h): the evaluation writes one bit per position and class, the runs, their joining
 * and the filter are counted, scanned and scattered from those bits, and a second evaluation of the tiles that hold a flagged
 * position adds the sums.  MFX_E_INVAL: a null argument, kstar not finite or <= 0, a sharded index, a sequence object that
 * holds a part only, evaluator and sequence on different devices; MFX_E_NOMEM: the planes or the runs do not fit the device. */
int  mfx_regions_run(mfx_eval *ev, const mfx_seq *seq, const mfx_regions_opts *o, mfx_regions **out, uint64_t *kasm, uint64_t *kmissing);
/* The result object (no reference seam: the reference writes -dump text, merfin-dump.C:70-79, and leaves the intervals to awk).  count:
 * its records; tiles_revisited: the tiles pass 2 evaluated (0 when no record survived); copy: the records in their order into dst[cap],
 * MFX_E_INVAL when cap is below count; free: releases it (NULL is fine). */
uint64_t mfx_regions_count(const mfx_regions *r);
uint64_t mfx_regions_tiles_revisited(const mfx_regions *r);
int  mfx_regions_copy(const mfx_regions *r, mfx_region *dst, uint64_t cap);
void mfx_regions_free(mfx_regions *r);
/* Diagnostic (tools/regions_rate.py; not part of the stable surface, like mfx_diag_spectrum_time): ms[3] = what the run spent in pass 1,
 * in runs / joining / filter, and in pass 2 (wall milliseconds, each waited for) */
void mfx_diag_regions_times(const mfx_regions *r, double *ms);
/* Host only (merfin-dump.C:70-79 writes one line per k-mer; this writes one per interval).  One header line, "#chrom start end class n_kmers mean_readK mean_asmK ext_kstar" (tab-separated), then one BED
 * line per record: the name (up to the first blank), the BASE span [start, end - 1 + k) -- a valid k-mer fits its contig, so
 * the span does -- the class by name, n_kmers, sum_readK / n_kmers, sum_asmK / n_kmers and ext_kstar, each "%.2f".  .gz / .bz2 /
 * .xz names go through the compressed writers (merfin-histogram.C:151). */
int  mfx_regions_write(const mfx_region *r, uint64_t n, const mfx_seq *seq, const char *const *names, int k, const char *bed_path);
/* Host only (tests, tools/native/regions_sanitize.cpp): the steps between the two passes -- starts and ends per word, count,
 * scan, scatter, joining by o->gap, filter by o->min_kmers, order -- over caller-made planes[3][ntiles * 64] of contigs of
 * contig_len[] positions (a contig takes ceil(len / 4096) tiles of 64 words per class; bit b of word w of a tile is position
 * 64 w + b; bits beyond a contig's end must be 0: MFX_E_INVAL).  The sums and ext_kstar of the records are 0; at most cap are
 * stored, *n_out counts them all.  o->kstar is not looked at. */
int  mfx_regions_from_planes_host(const uint64_t *planes, const uint64_t *contig_len, uint32_t ncontigs, const mfx_regions_opts *o,
                                  mfx_region *out, uint64_t cap, uint64_t *n_out);

/* ------------------------------------------------------------------------ */
/* -phase: hap-mer markers of two parents, their phase blocks and switch     */
/* errors, made on the device.  No reference counterpart: merfin has no trio */
/* mode.  The block rule is this project's own, in the spirit of Merqury's   */
/* phase blocks (its defaults, 100 switches within 20000 bases, are kept),   */
/* and is NOT validated against Merqury.                                     */
/* ------------------------------------------------------------------------ */
/* The index holds set A on its read side and set B on its assembly side (the sequence-only index: the k-mers of the sequence
 * claimed, A and B loaded update-only; any other index whose two values are > 0 exactly for A and for B gives the same records).
 * A k-mer start position is a MARKER of haplotype 0 when its k-mer is in A and not in B, of haplotype 1 when in B and not in A;
 * a k-mer in both is shared and no marker.  The markers of a contig in ascending order form RUNS: maximal stretches of
 * consecutive markers of one haplotype (positions without a marker are transparent).  A run of n markers whose first and last
 * lie at `first` and `last` spans last - first + k bases; it is SHORT iff n <= switches and span <= range, else LONG (with
 * switches = 0 every run is long).  A BLOCK opens at a contig's first run and at every long run whose nearest earlier long run
 * of the contig has the other haplotype; every other run joins the open block.  A block's haplotype is that of its long runs;
 * a block without a long run (then the contig's only block) takes the haplotype with more markers, a tie goes to 0.
 * Records are ordered by contig, start; every field is an integer.  48 bytes. */
typedef struct mfx_phase_block {
  uint32_t contig, hap;
  uint64_t start, end;       /* k-mer start positions: first marker, last marker + 1; the base span is [start, end - 1 + k) */
  uint64_t n_hap, n_switch;  /* markers of the block's own and of the other haplotype                                       */
  uint64_t n_switch_runs;    /* runs of the other haplotype in the block                                                     */
} mfx_phase_block;
typedef struct { uint64_t switches, range; } mfx_phase_opts;  /* -switches (100), -range (20000): any values are valid */
typedef struct mfx_phase mfx_phase;                           /* the result, held by the library */
/* The blocks of the whole sequence set into *out (release with mfx_phase_free).  Two passes (csrc/mfx_phase.h): the evaluation
 * writes one bit per position and haplotype and the per-contig totals; runs and blocks are counted, scanned and scattered from
 * those bits -- no atomic orders anything, a second run gives the same bytes.  The evaluator's K* parameters are not read.
 * MFX_E_INVAL: a null argument, a sharded index, a sequence object that holds a part only, evaluator and sequence on different
 * devices; MFX_E_NOMEM: the planes or the runs do not fit the device. */
int  mfx_phase_run(mfx_eval *ev, const mfx_seq *seq, const mfx_phase_opts *o, mfx_phase **out);
uint64_t mfx_phase_count(const mfx_phase *p);
int  mfx_phase_copy(const mfx_phase *p, mfx_phase_block *dst, uint64_t cap);
/* dst[ncontigs][4]: valid k-mers, A markers, B markers, shared k-mers of every contig; MFX_E_INVAL when cap (in contigs) is too small */
int  mfx_phase_contig_counts(const mfx_phase *p, uint64_t *dst, uint64_t cap);
void mfx_phase_free(mfx_phase *p);
/* Diagnostic (tools/phase_rate.py; not part of the stable surface): ms[2] = what the run spent in pass 1 and in runs / blocks */
void mfx_diag_phase_times(const mfx_phase *p, double *ms);
/* Host only.  Three texts (.gz / .bz2 / .xz stems compress each; the suffix stays last):
 *   <stem>.phased_block.bed    "#chrom start end hap n_hap n_switch n_switch_runs" (tab-separated), hap as A / B, the BASE span
 *   <stem>.hapmers.count       "#chrom A B shared kmers": one line per contig of contig_counts[ncontigs][4]
 *   <stem>.phased_block.stats  for A, B and all: blocks, sum / min / mean / max of the base spans, N50 (the largest L such that
 *                              blocks of span >= L hold at least half the sum), markers, switch markers, switch rate "%.6f"
 * names[c]: the contig names (up to the first blank). */
int  mfx_phase_write(const mfx_phase_block *b, uint64_t n, const uint64_t *contig_counts, const mfx_seq *seq, const char *const *names, int k,
                     const mfx_phase_opts *o, const char *stem);
/* Host only (tests, tools/native/phase_sanitize.cpp): pass 2 over caller-made planes[2][ntiles * 64] of contigs of contig_len[]
 * positions, laid out as for mfx_regions_from_planes_host; bits beyond a contig's end and a position in both planes: MFX_E_INVAL.
 * At most cap records are stored, *n_out counts them all. */
int  mfx_phase_from_planes_host(const uint64_t *planes, const uint64_t *contig_len, uint32_t ncontigs, int k, const mfx_phase_opts *o,
                                mfx_phase_block *out, uint64_t cap, uint64_t *n_out);

/* ------------------------------------------------------------------------ */
/* -bin: per-read hap-mer counts on the device, reads sorted by parent (trio */
/* binning).  No reference counterpart: merfin has no trio mode.  The class  */
/* rule is this project's own, in the spirit of Canu's haplotype split, and  */
/* is NOT validated against Canu.                                            */
/* ------------------------------------------------------------------------ */
/* The index behind the evaluator holds set A on its read side and set B on its assembly side, as for -phase; membership is
 * "value > 0".  Every record (read) gets the number of its valid k-mers, of those in A only, in B only and in both:
 * kmers = a + b + shared + in neither.  16 bytes. */
typedef struct mfx_bin_record { uint32_t kmers, a, b, shared; } mfx_bin_record;
typedef struct { uint64_t reads, bases, kmers, a, b, shared; double seconds_kernel, seconds_copy; } mfx_bin_stats;
typedef struct mfx_bin mfx_bin;
/* Records are batched as the read counters batch them (batch_bases per batch, 0: the library's; a record longer than the room left
 * is cut with a k - 1 overlap), packed into one of two pinned stages and counted on that stage's stream; the counts of the batch's
 * pieces of records come back on the same stream and are folded into the records in input order.  Integer sums only: a second run
 * gives the same bytes.  The evaluator's K* parameters are not read.  MFX_E_INVAL: a null argument, k > 31, a sharded index, a
 * batch below 2k + 2 bases. */
mfx_bin *mfx_bin_begin(mfx_eval *ev, uint64_t batch_bases);
/* n records; returns once bases / lens may be reused.  MFX_E_INVAL: a null argument, a record of 2^32 bases or more (nothing of the
 * call is taken then). */
int  mfx_bin_add(mfx_bin *b, const char *const *bases, const uint64_t *lens, uint64_t n);
/* sends the open batch and waits for every stage: every record added is final afterwards */
int  mfx_bin_flush(mfx_bin *b);
/* records whose counts are final and not yet taken.  A record is final when the stage that holds its last piece has settled (stages
 * settle inside add, flush and end); one shorter than k is final with zeros but keeps its place in the order. */
uint64_t mfx_bin_ready(const mfx_bin *b);
/* the next min(cap, ready) records, in input order */
int  mfx_bin_take(mfx_bin *b, mfx_bin_record *dst, uint64_t cap, uint64_t *n_out);
/* flushes and frees b whatever the result; records not taken are lost (the statistics count them) */
int  mfx_bin_end(mfx_bin *b, mfx_bin_stats *out);
/* The class rule, host only, integers only.  With NA = norm_a ? norm_a : 1 and NB likewise, a record is class 0 (A) iff
 * a + b >= min_hits and a * NB * 1000 > b * NA * ratio_milli, class 1 (B) iff the same holds with the roles swapped, else class 2
 * (unknown: ties, a = b = 0); the products in 128 bits.  MFX_E_INVAL: a null argument, ratio_milli < 1000 (both could hold). */
typedef struct { uint64_t norm_a, norm_b; uint32_t ratio_milli; uint32_t min_hits; } mfx_bin_opts;
int  mfx_bin_classify(const mfx_bin_record *r, uint64_t n, const mfx_bin_opts *o, uint8_t *cls);
/* Host only (tests, tools/native/bin_sanitize.cpp): the pieces n records of lens[] bases are cut into, batch after batch, by the
 * code the device path cuts with (csrc/mfx_bin.h) -- pieces[i] = batch, record, first position in the batch, length.  At most cap
 * are stored, *n_pieces counts them all.  batch_bases 0: the library's. */
int  mfx_bin_plan_host(const uint64_t *lens, uint64_t n, int k, uint64_t batch_bases, uint64_t *pieces, uint64_t cap, uint64_t *n_pieces);

/* ------------------------------------------------------------------------ */
/* -filter / -polish / -better / -strict / -loose: replaces processVariants */
/* + outputVariants (merfin-variants.C:131-345), vcfFile (vcf.C) and varMer  */
/* (varMer.C).  The host enumerates the allele-combination paths of many     */
/* clusters, the GPU scores every k-mer of every path in one launch of the   */
/* -dump lookup kernel, the host applies the mode's selector.                */
/* ------------------------------------------------------------------------ */
#define MFX_VAR_FILTER 4      /* OP_FILTER .. OP_LOOSE, merfin-globals.H:34-38 */
#define MFX_VAR_POLISH 5
#define MFX_VAR_BETTER 6
#define MFX_VAR_STRICT 7
#define MFX_VAR_LOOSE  8
typedef struct {
  int         mode;         /* MFX_VAR_*                                       */
  uint32_t    comb;         /* -comb (0 = default 15), merfin.C:144-145        */
  int         nosplit;      /* -nosplit                                        */
  const char *debug_path;   /* -debug log (merfin-variants.C:240-276) or NULL; */
                            /* a name ending in .gz is gzip-compressed         */
} mfx_variant_opts;
/* names/bases/lens: the contigs of -sequence (ident() = first header token is
 * matched against VCF CHROM, merfin-variants.C:141).  Writes headers + the
 * selected records to out_path (contigs in input order).  log_path receives
 * the PANIC / WARNING / progress lines (NULL = stderr). */
int mfx_variants_run(mfx_eval *ev, const char *vcf_path, const char *const *names, const char *const *bases,
                     const uint64_t *lens, uint32_t ncontigs, const mfx_variant_opts *opts,
                     const char *out_path, const char *log_path, uint64_t *n_clusters);
/* The VCF of a run read and parsed ahead of it (vcfFile::loadFile, vcf.C:93-149): host work only -- no device, no index --
 * so a caller runs it on a thread of its own under the index build (merfin opens the VCF after load_Kmers,
 * merfin-globals.C:201-219).  A handle serves ONE mfx_variants_run_vcf (clustering rearranges it); NULL on error.
 * mfx_variants_run_vcf = mfx_variants_run on the loaded records: same outputs, byte for byte. */
typedef struct mfx_vcf mfx_vcf;
mfx_vcf *mfx_vcf_load(const char *vcf_path);
void     mfx_vcf_free(mfx_vcf *vcf);
int mfx_variants_run_vcf(mfx_eval *ev, mfx_vcf *vcf, const char *const *names, const char *const *bases,
                         const uint64_t *lens, uint32_t ncontigs, const mfx_variant_opts *opts,
                         const char *out_path, const char *log_path, uint64_t *n_clusters);
/* Stage A of the variant modes ahead of the run, on a loaded VCF: the clusters merged for k (vcfFile::mergeChrPosGT, vcf.C:156-246) and
 * their allele combinations enumerated and packed batch by batch (merfin-variants.C:22-126, varMer.C:39) -- host work that needs the VCF
 * and the sequences but neither the index nor a device (merfin does it after load_Kmers, merfin-variants.C:131-230; here a caller runs it
 * under its index build).  The run -- mfx_variants_run_vcf on the same handle with the same sequences, k (the index's), opts->comb and
 * opts->nosplit: anything else is refused -- then starts at the lookups; its outputs are the unprepared run's byte for byte.  The
 * sequences must stay where they are until the run is over.  Once per handle. */
int mfx_vcf_prepare(mfx_vcf *vcf, int k, const char *const *names, const char *const *bases, const uint64_t *lens,
                    uint32_t ncontigs, const mfx_variant_opts *opts);
/* The PATH-ONLY index of the variant modes (round 6).  varMer::score (varMer.C:76-84) is the only place the variant modes ask the lookup
 * tables anything, and what it asks for are the k-mers of the enumerated paths; the reference nevertheless loads both databases whole
 * (load_Kmers, merfin-globals.C:114-163).  A prepared call set knows every path before a database is opened:
 *   mfx_vcf_prepare(vcf, k, ...);  mfx_vcf_path_bound(vcf, &n);            -- n: k-mer positions of all path text >= their distinct k-mers
 *   ix = mfx_index_create_for_seq(k, n + 1024, max_gb, device);
 *   mfx_index_claim_paths(ix, vcf, NULL);                                   -- the paths made on the device as the run makes them, their k-mers claimed
 *   mfx_index_load_db(ix, seqmers, 1, ...)  (or mfx_index_count_claimed(ix, assembly, 0));   mfx_index_load_db(ix, readmers, 0, minV, maxV);
 *   ev = mfx_eval_create(ix, ...);  mfx_variants_run_vcf(ev, vcf, ...);     -- same records, byte for byte, as on the full index
 * Both databases only UPDATE the claimed k-mers (a k-mer of no path never gets a slot).  The index is bound to the handle: another call set,
 * an unprepared run, -hist / -dump of a sequence are refused on it (MFX_E_INVAL).  k <= 31; a non-canonical database makes the load
 * return MFX_E_NONCANON as for every sequence-only index (build the full one). */
int mfx_vcf_path_bound(const mfx_vcf *vcf, uint64_t *positions);
int mfx_index_claim_paths(mfx_index *ix, mfx_vcf *vcf, uint64_t *n_positions);
/* The three steps above as ONE pass (what `merfin` does): the table is made as soon as the clusters are merged and every batch's k-mers are
 * claimed on the device while the host prepares the next batch.  *out: the claimed index, or NULL (with MFX_OK: the handle is prepared and runs
 * on a full index) when this call set cannot have one -- no memory for the table, a cluster the device cannot enumerate; mfx_last_error says why.
 * load_factor 0: the library's choice. */
int mfx_vcf_prepare_path_index(mfx_vcf *vcf, int k, const char *const *names, const char *const *bases, const uint64_t *lens, uint32_t ncontigs,
                               const mfx_variant_opts *opts, double max_gb, int device, double load_factor, mfx_index **out);
/* The same over an index sharded across nslots evaluators (slot d = shard d of nslots): every batch of path text is
 * scored by mfx_dump_values_sharded; clustering, enumeration, selectors and output are the code above. */
int mfx_variants_run_sharded(mfx_eval *const *evs, uint32_t nslots, const char *vcf_path, const char *const *names,
                             const char *const *bases, const uint64_t *lens, uint32_t ncontigs,
                             const mfx_variant_opts *opts, const char *out_path, const char *log_path,
                             uint64_t *n_clusters);

/* ------------------------------------------------------------------------ */
/* -completeness: replaces computeCompleteness (merfin-completeness.C:48-144)*/
/* as one streaming pass over the joint table.                              */
/* ------------------------------------------------------------------------ */
int mfx_completeness(mfx_eval *ev, double *total, double *undrcpy);
/* the 64 per-piece sums the reference prints (piece = top 6 bits of the k-mer = meryl file number,
 * merfin-completeness.C:56-66,119-120); arrays of 64 doubles each */
int mfx_completeness_pieces(mfx_eval *ev, double *total64, double *undrcpy64);

/* ------------------------------------------------------------------------ */
/* -spectrum / -peak auto: the copy-number spectrum of an index.  No seam of  */
/* the reference: merfin takes -peak from a k-mer multiplicity histogram of   */
/* the read database made outside it (meryl histogram -> GenomeScope).  Here  */
/* the 2-D histogram of the table's (read count, assembly count) pairs is one */
/* streaming pass over the table, and its single-copy row gives the peak.     */
/* ------------------------------------------------------------------------ */
#define MFX_E_NODATA     -10  /* the data holds no answer (mfx_spectrum_peak: no peak in the row) */
/* out: (copies + 2) x (max_mult + 1) cells, row-major.  Row r <= copies: entries whose assembly count is r; row copies + 1:
 * assembly count > copies.  Column m < max_mult: read count m; column max_mult: read count >= max_mult.  An entry is counted
 * once, with the counts mfx_index_value answers for its k-mer (the read count through the index's -min / -max filter, 0
 * outside it); an entry whose two counts are both 0 is not counted.  *n_entries: the counted entries = the sum of the image.
 * Every index form (a shard gives the spectrum of what it owns; a read-counted index that of its counted reads).
 * MFX_E_INVAL: copies outside [1, 6], max_mult outside [4, 65536], or an index that took non-canonical inserts (such a
 * database splits one k-mer over two entries: the spectrum of entries is not the spectrum of k-mers). */
int mfx_spectrum_run(const mfx_index *ix, uint32_t copies, uint32_t max_mult, uint64_t *out, uint64_t *n_entries);
/* Diagnostic (tools/spectrum_rate.py): the same pass `reps` times with the plain (aggregate 0) or the wave-aggregated (1) form of the
 * kernel, the time of each between two HIP events into kernel_ms[reps]; the image is checked against its entry count and dropped. */
int mfx_diag_spectrum_time(const mfx_index *ix, uint32_t copies, uint32_t max_mult, int aggregate, uint32_t reps, float *kernel_ms);
typedef struct {
  uint32_t valley;          /* first multiplicity at which the smoothed row stops falling                              */
  uint32_t main_peak;       /* highest point of the smoothed row beyond the valley                                   */
  uint32_t haploid_peak;    /* main_peak, or the peak at half of it where the 2-copy peak dominates: what -peak takes  */
  uint64_t count_at_peak;   /* row[haploid_peak]                                                                     */
} mfx_spectrum_peak_t;
/* Host only, exact integer arithmetic on one row of max_mult + 1 cells (column 0 and the overflow column take no part).
 * a[m], 1 <= m < max_mult: the mean of row[j] over j in [max(1, m-2), min(max_mult-1, m+2)], compared as rationals.
 * valley v: the smallest m in [1, max_mult-2] with a[m] <= a[m+1]; main peak p: the m in (v, max_mult) with the largest a[m]
 * (the smallest on ties); h: the m in [max(v+1, ceil(0.4 p)), floor(0.6 p)] with the largest a[m] (the smallest on ties);
 * the haploid peak is h when that range is not empty, 10 a[h] >= a[p] and a[h] >= a[j] for every j within 2 of h, else p.
 * MFX_E_NODATA: no v, or a[p] == 0 (an empty or falling row, a peak too low to tell from the error slope): ask for -peak. */
int mfx_spectrum_peak(const uint64_t *row, uint32_t max_mult, mfx_spectrum_peak_t *out);
/* Host only.  "Copies\tkmer_multiplicity\tCount", then one line per non-zero cell in row-major order: "read-only" (row 0), "1" ..
 * "<copies>", ">copies" with the number filled in (the last row); m (the overflow column as max_mult); the count.
 * with_read_only == 0 leaves row 0 out (a sequence-only index holds no such k-mers).  .gz / .bz2 / .xz names go through the
 * compressed writers.  The layout is believed to be the one Merqury's spectra-cn plot reads; UNVALIDATED against Merqury. */
int mfx_spectrum_write(const uint64_t *img, uint32_t copies, uint32_t max_mult, int with_read_only, const char *path);

#ifdef __cplusplus
}
#endif
#endif /* MERFIN_AMD_H */
