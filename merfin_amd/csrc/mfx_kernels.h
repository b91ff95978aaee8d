// mfx_kernels.h -- kernel argument blocks and launch wrappers (mfx_kernels.hip)
#pragma once
#include "mfx_internal.h"

// K* parameters + accumulators shared by every histogram-producing kernel
struct mfx_kstar_args {
  double          peak;
  uint32_t        n_prob;
  const uint32_t *probK;
  const double   *probP;
  uint32_t        nbins;
  uint32_t        ncontigs;
  uint64_t       *counts;             // layout: include/merfin_amd.h MFX_HIST_WORDS
  double         *partials;           // [gridDim.x]
  uint64_t       *ovf;                // the evaluator's table of far K* bins (mfx_eval::d_ovf)
  const uint64_t *underq = nullptr;   // [MFX_MAXP_LDS * MFX_KLUT] mfx_kfix of the over-copy term of (read count, asmV) where the exact tables apply, else 0 (mfx_eval_create)
};

constexpr uint32_t MFX_WL_HEADER = 4096 + 2;    // words in front of the worklist's entries (<= 4096 segments)
struct mfx_hist_args {
  mfx_table_view  t;                  // t.compact: the 8-byte-slot layout of a sequence-only index (mfx_kernels.hip)
  int             canonical;          // 1: single probe of min(f,r); 0: probe both strands and sum
  const uint8_t  *bases;
  const uint64_t *codes = nullptr;    // non-null: read the tiles from the packed planes (same byte offsets / 32) instead of `bases`
  const uint32_t *valid = nullptr;
  const uint64_t *contig_off, *contig_len, *tile_start;
  uint32_t        ncontigs;
  uint64_t        tile_begin, tile_end;
  const uint32_t *tile_contig;        // [ntiles] contig of every tile
  uint64_t       *tile_ctr;           // dynamic tile scheduler: tiles handed out beyond the first gridDim.x (0 at launch)
  double         *tile_partials;      // [n_logical * MFX_BLOCK/64] koverCpy of every (tile, wave) of this launch
  // The launch evaluates n_logical tiles, numbered li = 0 .. n_logical-1:
  //   part_n == 1 : the contiguous range, tile = tile_begin + li
  //   part_n  > 1 : block-cyclic share of rank part_rank: tile = ((li >> part_shift) * part_n + part_rank << part_shift) + (li & mask)
  uint64_t        n_logical;
  uint32_t        part_rank, part_n, part_shift;
  uint64_t       *dbg = nullptr;      // non-null: the debug instance of the kernel counts the probe's endings here (mfx_eval_debug_counters)
  // the worklist of mfx_hist_rest_kernel (compact layout, canonical database; else null): words [2, 2 + wl_segs) = entries in each segment (one
  // per block of the main kernel's grid), from word MFX_WL_HEADER: 16-byte entries {k-mer, aux, slot | mode << 29 | dbl << 31}, segment g at g * wl_segcap
  uint64_t       *wl = nullptr;
  uint32_t        wl_segs = 0, wl_segcap = 0;
  mfx_kstar_args  ks;
};

struct mfx_route_args {
  mfx_table_view  t;
  const uint8_t  *bases;
  const uint64_t *contig_off, *contig_len, *tile_start;
  uint32_t        ncontigs;
  uint64_t        tile_begin, tile_end;
  uint32_t        nranks;
  uint64_t       *keys;               // [ntiles * MFX_TILE] canonical k-mer per position (~0: none)
  uint8_t        *owner;              // [ntiles * MFX_TILE] owner rank (255: none)
  uint64_t       *dest_counts;        // [nranks]
  uint64_t       *counts;             // counts image: kasm + per-contig kasm are added here
  uint32_t        nbins;
  // direct split (nranks <= MFX_SPLIT_MAX_RANKS): no sort, no position-sized scratch
  const uint32_t *tile_contig;        // [ntiles of the sequence set]
  uint32_t       *tile_cnt;           // [(tile_end - tile_begin) * nranks] k-mers of each tile per owner; then, in place,
                                      //   their exclusive prefix over the tiles (per owner)
};

constexpr uint32_t MFX_KEYS_MAX_SEGS = 16;
struct mfx_hist_keys_args {
  mfx_table_view  t;
  const uint64_t *keys = nullptr;     // nseg == 0: one array of n k-mers with their contigs; koverCpy as ordered fp64 partials (ks.partials)
  const uint32_t *contig = nullptr;
  uint64_t        n = 0;              // k-mers in all (nseg > 0: the sum of seg_n)
  // nseg > 0: the k-mers as segments, evaluated where they lie; koverCpy in fixed point (units of 2^-52) into kfix[0..1] (low, high word)
  uint32_t        nseg = 0;
  const uint64_t *seg_keys[MFX_KEYS_MAX_SEGS] = {};
  const uint32_t *seg_contig[MFX_KEYS_MAX_SEGS] = {};
  uint64_t        seg_n[MFX_KEYS_MAX_SEGS] = {};
  uint64_t       *kfix = nullptr;
  mfx_kstar_args  ks;
};

struct mfx_dump_args {
  mfx_table_view  t;
  int             canonical;
  const uint8_t  *src;         // contig base + first tile offset (128-byte aligned)
  uint64_t        npos;        // start positions to evaluate from src (tile-aligned begin)
  uint64_t        skip;        // first `skip` positions are not written (pos_begin % TILE)
  uint64_t        clen_left;   // contig bases remaining from src
  uint32_t       *readV, *asmV;// device output, index = position - skip
  double          peak;
  uint32_t        n_prob;
  const uint32_t *probK;
  const double   *probP;
  uint64_t       *stats;       // [0] kasm [1] kmissing
  int             recount = 0; // 1: readV holds final values; only the counters are taken again (sharded index)
};

// -track (mfx_track_kernel / mfx_w_track_kernel; csrc/mfx_track.h): the whole sequence set, tile by tile
struct mfx_track_args {
  mfx_table_view  t;
  int             canonical;
  const uint8_t  *bases;
  const uint64_t *codes = nullptr;    // non-null (k <= 31): the tiles are read from the packed planes, as -hist does
  const uint32_t *valid = nullptr;
  const uint64_t *contig_off, *contig_len, *tile_start;
  const uint32_t *tile_contig;
  const uint64_t *contig_rec;         // [ncontigs] number of the first window record of each contig
  uint64_t        ntiles;
  uint64_t        window;             // start positions per window (>= 1)
  double          peak;
  uint32_t        n_prob;
  const uint32_t *probK;
  const double   *probP;
  uint64_t       *recs;               // the records: 9 words each (mfx_track_window), zero at launch
  uint64_t       *stats;              // [0] kasm [1] kmissing
};

// -regions (csrc/mfx_regions.h).  Pass 1 (mfx_regions_class_kernel / mfx_w_regions_class_kernel) writes the class planes and the two totals;
// pass 2 (mfx_regions_sums_kernel / mfx_w_regions_sums_kernel) evaluates the flagged positions of the flagged tiles again for the sums
struct mfx_regions_args {
  mfx_table_view  t;
  int             canonical;
  const uint8_t  *bases;
  const uint64_t *codes = nullptr;    // non-null (k <= 31): the tiles are read from the packed planes, as -hist does
  const uint32_t *valid = nullptr;
  const uint64_t *contig_off, *contig_len, *tile_start;
  const uint32_t *tile_contig;
  uint64_t        ntiles;
  double          peak;
  uint32_t        n_prob;
  const uint32_t *probK;
  const double   *probP;
  double          kstar;              // the threshold t: finite, > 0
  uint64_t       *planes;             // [3][ntiles * 64]: bit b of word tile * 64 + w = position 64 w + b of the tile; every word is written by pass 1
  uint64_t       *stats = nullptr;    // pass 1: [0] kasm [1] kmissing
  // pass 2
  const uint64_t *tile_flag = nullptr;   // [ntiles] != 0: one of the tile's 192 plane words is not 0
  uint64_t       *regs = nullptr;     // the records, 7 words each (mfx_region), class after class, each class in (contig, start) order;
                                      //   word 6 holds the largest key (collapsed) / ~key (expanded) of K* while the kernel runs
  uint64_t       *recount = nullptr;  // [records] the flagged k-mers pass 2 found for each
  uint64_t        reg_begin0 = 0, reg_begin1 = 0, reg_begin2 = 0, reg_begin3 = 0;   // class c's records: [reg_begin c, reg_begin c+1)
};

// -phase (csrc/mfx_phase.h).  Pass 1 (mfx_phase_mark_kernel / mfx_w_phase_mark_kernel) writes the two haplotype planes and the per-contig totals
struct mfx_phase_args {
  mfx_table_view  t;
  int             canonical;
  const uint8_t  *bases;
  const uint64_t *codes = nullptr;    // non-null (k <= 31): the tiles are read from the packed planes, as -hist does
  const uint32_t *valid = nullptr;
  const uint64_t *contig_off, *contig_len, *tile_start;
  const uint32_t *tile_contig;
  uint64_t        ntiles;
  uint64_t       *planes;             // [2][ntiles * 64]: plane 0 in A and not in B, plane 1 in B and not in A; every word is written
  uint64_t       *counts;             // [ncontigs][4] += valid k-mers, A markers, B markers, shared; zero at launch
};

// -bin (csrc/mfx_bin.h; mfx_bin_kernel, k <= 31): one batch of reads as mfx_reads_args has it, and the batch's pieces
struct mfx_bin_args {
  mfx_table_view  t;
  int             canonical;
  const uint64_t *codes;
  const uint32_t *valid;
  uint64_t        npos;               // base positions of the batch (separators included)
  const uint64_t *piece_start;        // [npieces] first position of every piece, ascending
  const uint64_t *tile_first;         // [tiles] the first piece that touches the tile (npieces: none)
  uint64_t        npieces;
  uint64_t       *out;                // [npieces][2] += k-mers | A only << 32, B only | shared << 32 (mfx_bin_record as two words); zero at launch
};

struct mfx_count_args {
  mfx_table_view  t;
  const uint8_t  *bases;
  const uint64_t *codes = nullptr;    // the sequence's packed planes (2-bit codes, validity bits): read instead of `bases` when given
  const uint32_t *valid = nullptr;
  const uint64_t *contig_off, *contig_len, *tile_start;
  uint32_t        ncontigs;
  uint64_t        ntiles;
  uint64_t       *meta;
  int             count = 1;          // 1: asmV += 1 per occurrence (`meryl count`); 0: claim the k-mers only (sequence-only index); 2: asmV += 1 for the k-mers claimed BEFORE, no claims
};

// one batch of reads for the read k-mer counter (mfx_reads_kernel / mfx_w_reads_kernel): the planes of mfx_pack_bases, reads back to
// back with one invalid base between two; room for whole tiles + the halo ((npos + MFX_TILE - 1) / MFX_TILE * 128 + MFX_TILE_WORDS words,
// invalid beyond npos)
struct mfx_reads_args {
  mfx_table_view  t;
  const uint64_t *codes;
  const uint32_t *valid;
  uint64_t        npos;               // base positions of the batch (separators included)
  uint64_t       *meta;               // the index's meta words (side-table claims that hit the probe limit: [2])
  uint64_t       *stats;              // [4] += valid k-mers, k-mers added to a claimed k-mer, k-mers dropped, k-mers whose read count moved to the side table (or arrived in it)
  uint64_t        key_lo = 0, key_hi = 0;   // mfx_k_reads_claim_range only: the k-mers with key_lo <= key < key_hi are counted
};

// varMer::score of the paths of a batch (mfx_var_score_kernel): everything device memory
struct mfx_var_score_args {
  const uint8_t  *text;               // the packed path text (every path followed by '\n')
  const uint32_t *readV, *asmV;       // per start position of the text (mfx_dump_kernel)
  uint64_t        npaths;
  const uint64_t *off;                // [npaths] first base of the path in `text`
  const uint32_t *len, *nv;           // [npaths] bases; variants of its cluster
  const uint64_t *voff;               // [npaths] first of its nv entries in gt / vidx / vlen
  const uint64_t *cfirst;             // [npaths] number of the first path of its cluster
  const int32_t  *gt;
  const uint32_t *vidx, *vlen;
  uint32_t        k;
  int             need_dk;            // 0: numM only (-filter / -better / -strict / -loose), 1: + totdk (-polish)
  double          peak;
  uint32_t        n_prob;
  const uint32_t *probK;
  const double   *probP;
  uint32_t       *numM;               // [npaths] out
  double         *totdk;              // [npaths] out (need_dk)
};
hipError_t mfx_k_var_score(const mfx_var_score_args &a, hipStream_t st);
hipError_t mfx_k_var_traverse(const mfx_trv_cluster *cl, uint64_t ncl, const mfx_trv_variant *vars, const mfx_trv_allele *alleles, const char *win_text,
                              const char *allele_text, const mfx_trv_out &o, uint32_t *np, uint32_t *status, hipStream_t st);
hipError_t mfx_k_table_init(mfx_slot *slots, uint64_t nslots, hipStream_t st);
hipError_t mfx_k_table_add(mfx_table_view t, const uint64_t *kmers, const uint32_t *values, uint64_t n, int side,
                           uint64_t *meta, hipStream_t st);
// delta-coded blocks (mfx_db.cpp FLAT_DELTA): dir = {first k-mer, byte offset | kbits << 48 | vbits << 56} per block + one closing
// entry; payload_base = the file offset payload[0] holds; n = k-mers of the nblocks blocks
hipError_t mfx_k_table_add_delta(mfx_table_view t, const uint64_t *payload, const uint64_t *dir, uint32_t nblocks, uint64_t n,
                                 uint64_t payload_base, int side, uint64_t *meta, hipStream_t st);
// a PLACED database's blocks (records = the numbers P of mfx_place.h, ascending: the order of the table's lines)
hipError_t mfx_k_table_add_placed(mfx_table_view t, const uint64_t *payload, const uint64_t *dir, uint32_t nblocks, uint64_t n,
                                  uint64_t payload_base, int side, uint64_t *meta, hipStream_t st);
int        mfx_k_table_takes_placed(const mfx_table_view &t);
hipError_t mfx_k_place_keys(int k, const uint64_t *kmers, uint64_t n, uint64_t *out, hipStream_t st);
hipError_t mfx_k_table_value(mfx_table_view t, const uint64_t *kmers, uint64_t n, uint32_t *readV, uint32_t *asmV,
                             hipStream_t st);
hipError_t mfx_k_table_export(mfx_table_view t, uint64_t *kmers, uint32_t *readV, uint32_t *asmV,
                              unsigned long long *count, hipStream_t st);
hipError_t mfx_k_hist(const mfx_hist_args &a, int grid, hipStream_t st);
hipError_t mfx_k_route(const mfx_route_args &a, hipStream_t st);
hipError_t mfx_k_route_split(const mfx_route_args &a, uint64_t *keys_out, uint32_t *contig_out, hipStream_t st);
hipError_t mfx_k_route_gather(const mfx_route_args &a, const uint32_t *idx, uint64_t nvalid, uint64_t *keys_out,
                              uint32_t *contig_out, hipStream_t st);
hipError_t mfx_k_iota(uint32_t *v, uint64_t n, hipStream_t st);
hipError_t mfx_k_hist_keys(const mfx_hist_keys_args &a, int grid, hipStream_t st);
// one-pass router (atomic reservation per tile and owner): owner d's k-mers at keys_out[d * region_cap ...), cursors[d] of them; cursors[nranks] != 0: a region overflowed
hipError_t mfx_k_route_fused(const mfx_route_args &a, uint64_t *keys_out, uint32_t *contig_out, uint64_t *cursors, uint64_t region_cap, hipStream_t st);
hipError_t mfx_k_sum_partials(const double *partials, uint32_t n, double *out, hipStream_t st);
hipError_t mfx_k_ordered_sum(const double *v, uint32_t n, double *out, hipStream_t st);
uint64_t mfx_k_tile_partials_words(uint64_t ntiles);
hipError_t mfx_k_sum_tile_partials(double *tile_partials, uint64_t ntiles, double *out, uint64_t *ctr_reset, hipStream_t st, int fixed);   // fixed: the values are integers, units of 2^-52 (k <= 31)
hipError_t mfx_k_hist_rest(const mfx_hist_args &a, int grid, hipStream_t st);
int mfx_k_hist_resident_blocks(int compact, int k);
int mfx_k_quot_supported();
hipError_t mfx_k_gather_rate(const void *table, uint64_t nlines, uint64_t *scratch, double *lines_per_s, hipStream_t st);
// 32 <= k <= 64 (mfx_wide.hip); kmers: two uint64 words per k-mer {low 64 bits, high bits}
hipError_t mfx_kw_table_add(mfx_table_view t, const uint64_t *kmers, const uint32_t *values, uint64_t n, int side, uint64_t *meta, hipStream_t st);
hipError_t mfx_kw_table_value(mfx_table_view t, const uint64_t *kmers, uint64_t n, uint32_t *readV, uint32_t *asmV, hipStream_t st);
hipError_t mfx_kw_table_export(mfx_table_view t, uint64_t *kmers, uint32_t *readV, uint32_t *asmV, unsigned long long *count, hipStream_t st);
hipError_t mfx_kw_hist(const mfx_hist_args &a, int grid, hipStream_t st);
hipError_t mfx_kw_dump(const mfx_dump_args &a, hipStream_t st);
hipError_t mfx_kw_count(const mfx_count_args &a, hipStream_t st);
hipError_t mfx_kw_completeness(mfx_table_view t, double peak, uint32_t n_prob, const uint32_t *probK, const double *probP, double *partials,
                               int grid, hipStream_t st);
hipError_t mfx_k_dump(const mfx_dump_args &a, hipStream_t st);
hipError_t mfx_k_track(const mfx_track_args &a, hipStream_t st);          // k <= 31
hipError_t mfx_kw_track(const mfx_track_args &a, hipStream_t st);         // 32 <= k <= 64 (mfx_wide.hip)
hipError_t mfx_k_regions_class(const mfx_regions_args &a, hipStream_t st);     // k <= 31
hipError_t mfx_kw_regions_class(const mfx_regions_args &a, hipStream_t st);    // 32 <= k <= 64 (mfx_wide.hip)
hipError_t mfx_k_regions_sums(const mfx_regions_args &a, hipStream_t st);
hipError_t mfx_kw_regions_sums(const mfx_regions_args &a, hipStream_t st);
// the steps between the passes (mfx_regions.hip); every array is the caller's, every count a uint64
size_t     mfx_k_rg_temp_bytes(uint64_t n);                                        // temporary storage the scan / the sum of n counts needs
hipError_t mfx_k_rg_scan(uint64_t *d, uint64_t n, void *tmp, size_t tmp_bytes, hipStream_t st);      // exclusive prefix sums, in place; waits for nothing
hipError_t mfx_k_rg_sum(const uint64_t *d, uint64_t n, uint64_t *out, void *tmp, size_t tmp_bytes, hipStream_t st);
hipError_t mfx_k_rg_pick(const uint64_t *src, const uint64_t *idx /* host */, uint32_t n /* <= 4 */, uint64_t *dst, hipStream_t st);   // dst[i] = src[idx[i]]
hipError_t mfx_k_rg_count(const uint64_t *planes, uint64_t ntiles, const uint32_t *tile_contig, uint64_t *cnt_s, uint64_t *cnt_e, uint64_t *tile_flag, hipStream_t st);
hipError_t mfx_k_rg_scatter(const uint64_t *planes, uint64_t ntiles, const uint64_t *tile_start, const uint32_t *tile_contig, const uint64_t *off_s,
                            const uint64_t *off_e, uint32_t *run_contig, uint64_t *run_start, uint64_t *run_end, hipStream_t st);
hipError_t mfx_k_rg_heads(const uint32_t *run_contig, const uint64_t *run_start, const uint64_t *run_end, uint64_t nruns, const uint64_t *cls_run /* [4], host */,
                          uint64_t gap, uint64_t *head, uint64_t *len, hipStream_t st);
hipError_t mfx_k_rg_bounds(const uint64_t *head_x /* exclusive scan of head, nruns + 1 */, uint64_t nruns, uint64_t *reg_first, uint64_t *reg_last, hipStream_t st);
hipError_t mfx_k_rg_keep(const uint64_t *reg_first, const uint64_t *reg_last, const uint64_t *len_x /* exclusive scan of len, nruns + 1 */, uint64_t nraw,
                         uint64_t min_kmers, uint64_t *keep, hipStream_t st);
hipError_t mfx_k_rg_emit(const uint64_t *reg_first, const uint64_t *reg_last, const uint64_t *len_x, const uint64_t *keep_x /* exclusive scan of keep, nraw + 1 */,
                         uint64_t nraw, const uint64_t *cls_run /* [4], host */, const uint32_t *run_contig, const uint64_t *run_start, const uint64_t *run_end,
                         uint64_t *regs, hipStream_t st);
hipError_t mfx_k_rg_finish(uint64_t *regs, uint64_t nreg, hipStream_t st);        // word 6: key -> ext_kstar
hipError_t mfx_k_phase_mark(const mfx_phase_args &a, hipStream_t st);          // k <= 31
hipError_t mfx_k_bin(const mfx_bin_args &a, hipStream_t st);                   // k <= 31
hipError_t mfx_kw_phase_mark(const mfx_phase_args &a, hipStream_t st);         // 32 <= k <= 64 (mfx_wide.hip)
// pass 2 of -phase (mfx_phase.hip); the sums are mfx_k_rg_scan's, the bounds mfx_k_rg_bounds'
size_t     mfx_k_ph_temp_bytes(uint64_t n);                                        // temporary storage any scan of n entries needs
hipError_t mfx_k_ph_join_scan(const uint64_t *in, uint64_t *out, uint64_t n, void *tmp, size_t tmp_bytes, hipStream_t st);   // inclusive, by mfx_ph_join
hipError_t mfx_k_ph_tile(const uint64_t *planes, uint64_t ntiles, const uint64_t *tile_start, const uint32_t *tile_contig, uint64_t *cnt /* ntiles + 1 */,
                         uint64_t *car /* ntiles */, hipStream_t st);
hipError_t mfx_k_ph_count(const uint64_t *planes, uint64_t ntiles, const uint64_t *tile_start, const uint32_t *tile_contig, const uint64_t *car /* scanned */,
                          uint64_t *cnt_run /* ntiles + 1 */, hipStream_t st);
hipError_t mfx_k_ph_scatter(const uint64_t *planes, uint64_t ntiles, const uint64_t *tile_start, const uint32_t *tile_contig, const uint64_t *car, const uint64_t *rank0,
                            const uint64_t *off, uint32_t *run_contig, uint32_t *run_hap, uint64_t *run_start, uint64_t *run_end, uint64_t *run_rank, hipStream_t st);
hipError_t mfx_k_ph_runs(const uint32_t *run_contig, const uint32_t *run_hap, const uint64_t *run_start, const uint64_t *run_end, const uint64_t *run_rank, uint64_t nruns,
                         uint64_t nmarkers, uint64_t k, uint64_t S, uint64_t R, uint64_t *lng /* nruns */, uint64_t *cnt_a /* nruns + 1 */, uint64_t *cnt_b, hipStream_t st);
hipError_t mfx_k_ph_heads(const uint32_t *run_contig, const uint32_t *run_hap, const uint64_t *lng, const uint64_t *lng_x, uint64_t nruns, uint64_t *head /* nruns + 1 */,
                          hipStream_t st);
hipError_t mfx_k_ph_emit(const uint64_t *blk_first, const uint64_t *blk_last, uint64_t nblocks, const uint32_t *run_contig, const uint32_t *run_hap,
                         const uint64_t *run_start, const uint64_t *run_end, const uint64_t *lng_x, const uint64_t *a_x, const uint64_t *b_x, uint64_t *recs, hipStream_t st);
hipError_t mfx_k_track_finish(uint64_t *recs, uint64_t nrec, hipStream_t st);   // the min / max keys of the records -> doubles (+inf / -inf where nothing was scored)
// *out += the content digest of nwords 32-base words (codes != nullptr: from the packed planes, else from the bytes)
hipError_t mfx_k_seq_digest(const uint8_t *bases, const uint64_t *codes, const uint32_t *valid, uint64_t nwords, uint64_t *out, hipStream_t st);
hipError_t mfx_k_add_u32(uint32_t *dst, const uint32_t *src, uint64_t n, hipStream_t st);
hipError_t mfx_k_pack(const uint8_t *bases, uint64_t *codes, uint32_t *valid, uint64_t nwords, hipStream_t st);
hipError_t mfx_k_unpack(const uint64_t *codes, const uint32_t *valid, uint8_t *bases, uint64_t nwords, hipStream_t st);
hipError_t mfx_k_valid_scatter(uint32_t *valid, const uint64_t *exc, uint32_t n, hipStream_t st);     // exc[i] = word index | word << 32
hipError_t mfx_k_count(const mfx_count_args &a, hipStream_t st);
hipError_t mfx_k_reads(const mfx_reads_args &a, hipStream_t st);        // k <= 31: sequence-only / path-only index (every layout)
hipError_t mfx_kw_reads(const mfx_reads_args &a, hipStream_t st);       // 32 <= k <= 64 (mfx_wide.hip)
hipError_t mfx_k_reads_claim(const mfx_reads_args &a, hipStream_t st);  // k <= 31, a full table of 16-byte slots: every k-mer is claimed if absent (mfx_reads_begin_all)
hipError_t mfx_k_reads_claim_range(const mfx_reads_args &a, hipStream_t st);   // ... only the k-mers of [a.key_lo, a.key_hi); the others add to stats[0] alone (mfx_reads_begin_range)
// every entry of a full table of 16-byte slots into the (empty) table nt; meta: nt's words, zero at launch ([0]: entries moved, [2]: probe-limit failures)
hipError_t mfx_k_table_rehash(const mfx_slot *old_slots, uint64_t old_nslots, mfx_table_view nt, uint64_t *meta, hipStream_t st);
// mfx_index_write_db (mfx_sort.hip): bins[key >> shift] += 1 for every entry whose count on `side` is non-zero
hipError_t mfx_k_db_bins(mfx_table_view t, int side, int shift, uint32_t nbins, uint64_t *bins, hipStream_t st);
// ... those of them with bin_lo <= key >> shift < bin_hi, compacted into keys / vals (at most cap; *count ends as their number, also beyond cap)
hipError_t mfx_k_db_export(mfx_table_view t, int side, int shift, uint32_t bin_lo, uint32_t bin_hi, uint64_t *keys, uint32_t *vals, uint64_t cap,
                           unsigned long long *count, hipStream_t st);
// ascending keys (bits [0, key_bits)) with their values; tmp == nullptr: only tmp_bytes is set
int mfx_sort_db_pairs(void *tmp, size_t &tmp_bytes, const uint64_t *kin, uint64_t *kout, const uint32_t *vin, uint32_t *vout, uint64_t n, int key_bits,
                      hipStream_t st);
// the encoder of the streamed database writer (mfx_sort.hip): full blocks of MFX_DELTA_BLOCK sorted pairs -> the words of mfx_db.cpp's pack_delta_block
struct mfx_delta_plan { uint64_t first; uint32_t widths, nesc; };      // per block: its first k-mer, kb | vb << 8 (mfx_delta.h), its escapes
hipError_t mfx_k_delta_plan(const uint64_t *keys, const uint32_t *vals, uint32_t nblocks, mfx_delta_plan *plan, hipStream_t st);
// word_off / esc_off: where block b's words start in out, its escapes in esc_keys / esc_vals -- the scan of the plan's sizes
hipError_t mfx_k_delta_pack(const uint64_t *keys, const uint32_t *vals, uint32_t nblocks, const mfx_delta_plan *plan, const uint64_t *word_off,
                            const uint32_t *esc_off, uint64_t *out, uint64_t *esc_keys, uint32_t *esc_vals, hipStream_t st);
// mfx_db_merge (mfx_merge.hip).  One block of one input in a window: its words at payload + word_off, its cnt records to keys / vals from
// `out` on; every k-mer of it lies below `limit` (the next block's first k-mer, or the end of the key space); [esc_lo, esc_hi): the
// window's slice of its input's escape list in esc_keys / esc_vals; input: which input the block is of
struct mfx_merge_task { uint64_t word_off, first, limit, out; uint32_t kb, vb, cnt, esc_lo, esc_hi, input; };
constexpr uint32_t MFX_MERGE_ERR_ORDER = 1u, MFX_MERGE_ERR_ESCAPE = 2u, MFX_MERGE_ERR_ZERO = 4u;      // err[input] of the decode: what no writer makes
// below[t] / above[t]: the records of task t under lo / at or above hi
hipError_t mfx_k_delta_decode(const mfx_merge_task *tasks, uint32_t ntasks, const uint64_t *payload, const uint64_t *esc_keys, const uint32_t *esc_vals, uint64_t lo,
                              uint64_t hi, uint64_t *keys, uint32_t *vals, uint32_t *below, uint32_t *above, uint32_t *err, hipStream_t st,
                              uint32_t zero_from = ~0u /* the inputs from this one on leave with a count of 0: mfx_db_merge_except */);
// two ascending runs into one of la + lb pairs; equal k-mers stay, a's first
hipError_t mfx_k_merge_pairs(const uint64_t *ka, const uint32_t *va, uint64_t la, const uint64_t *kb, const uint32_t *vb, uint64_t lb, uint64_t *ko, uint32_t *vo,
                             hipStream_t st);
// one record per k-mer of a merged run: op (MFX_MERGE_*), then the filter; tile_off: mfx_combine_tiles(n) + 1 words, the last ends as the number of
// records written; stats[0] += sums clamped, stats[1] += k-mers filtered
uint64_t mfx_combine_tiles(uint64_t n);
hipError_t mfx_k_combine(const uint64_t *keys, const uint32_t *vals, uint64_t n, uint32_t n_in, int op, uint64_t minV, uint64_t maxV, uint64_t *tile_off,
                         uint64_t *out_keys, uint32_t *out_vals, uint64_t *stats, hipStream_t st);
// mfx_db_join_* (mfx_join.hip): the sorted join of a read run a and an asm run b, both strictly ascending, into -completeness' piece sums
// (pieces[128], added to) or the -spectrum image (a.img, added to; a.t takes no part); stats[0] += the k-mers both runs hold.  grid: the
// persistent workgroups.
struct mfx_spectrum_args;
hipError_t mfx_k_join_completeness(const uint64_t *ka, const uint32_t *va, uint64_t la, const uint64_t *kb, const uint32_t *vb, uint64_t lb, int k, double peak,
                                   uint32_t n_prob, const uint32_t *probK, const double *probP, double *pieces, uint64_t *stats, int grid, hipStream_t st);
hipError_t mfx_k_join_spectrum(const uint64_t *ka, const uint32_t *va, uint64_t la, const uint64_t *kb, const uint32_t *vb, uint64_t lb, const mfx_spectrum_args &a,
                               uint64_t minV, uint64_t maxV, uint64_t *stats, int grid, hipStream_t st);
// mfx_db_trio, mfx_db_trio_hist, mfx_db_histogram (mfx_trio.hip; the rule: mfx_trio.h).  tag: the role into the two low bits of an input's decoded
// k-mers, in place.  hist: the three rows of a tagged merged run into a.img (a.copies == 1: 3 rows and the counter word, added to).  classify: the
// two hap-mer sets of a tagged merged run, ascending and dense, behind a_keys / b_keys; tile_off: 2 * (mfx_trio_tiles(n) + 1) words, the last two
// end as the k-mers written to A and to B; stats: MFX_TRIO_STAT_WORDS words (copies of the MFX_TRIO_S_* counters, mfx_trio.h), added to.
struct mfx_trio_cuts;
hipError_t mfx_k_trio_tag(uint64_t *keys, uint64_t n, uint32_t role, hipStream_t st);
hipError_t mfx_k_trio_hist(const uint64_t *keys, const uint32_t *vals, uint64_t n, const mfx_spectrum_args &a, int grid, hipStream_t st);
uint64_t mfx_trio_tiles(uint64_t n);
hipError_t mfx_k_trio_classify(const uint64_t *keys, const uint32_t *vals, uint64_t n, const mfx_trio_cuts &cuts, uint64_t *tile_off, uint64_t *a_keys, uint32_t *a_vals,
                               uint64_t *b_keys, uint32_t *b_vals, uint64_t *stats, hipStream_t st);
// mfx_db_diploid (mfx_diploid.hip; the rule: mfx_diploid.h).  pairs: the tagged merged run of hap1 and hap2 into the pair run -- one record
// (k-mer, c1 | c2 << 32) per k-mer, ascending and dense, room for n; tile_off: mfx_dip_tiles(n) + 1 words, the last ends as the records written.
// join: the read run a against the pair run; cls / cn: the class image (copies == 2) and the cn image, one lds_cols, each with its counter word
// behind it, added to; sums[256] (tot[64], und[3][64]; pieces != 0) and counters[MFX_DIP_STAT_WORDS] added to; stats[0] += the k-mers both hold.
uint64_t mfx_dip_tiles(uint64_t n);
hipError_t mfx_k_dip_pairs(const uint64_t *keys, const uint32_t *vals, uint64_t n, uint64_t *tile_off, uint64_t *pk, uint64_t *pv, hipStream_t st);
hipError_t mfx_k_dip_join(const uint64_t *ka, const uint32_t *va, uint64_t la, const uint64_t *pk, const uint64_t *pv, uint64_t lb, const mfx_spectrum_args &cls,
                          const mfx_spectrum_args &cn, uint64_t minV, uint64_t maxV, int k, int pieces, double peak, uint32_t n_prob, const uint32_t *probK,
                          const double *probP, double *sums, uint64_t *counters, uint64_t *stats, int grid, hipStream_t st);
hipError_t mfx_k_completeness(mfx_table_view t, double peak, uint32_t n_prob, const uint32_t *probK, const double *probP,
                              double *partials, int grid, hipStream_t st);
