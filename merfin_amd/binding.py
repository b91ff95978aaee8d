"""ctypes binding of include/merfin_amd.h.  Names follow the reference's
objects: Index <-> the merylExactLookup pair (merfin-globals.H:217,220),
Sequences <-> the dnaSeq records loadSequence produces (merfin.C:30-53),
Evaluator <-> merfinGlobal's K* parameters + process*/output* callbacks."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
TILE = 4096

MFX_ERRORS = {-1: "INVAL", -2: "NOMEM", -3: "HIP", -4: "FULL", -5: "OVERFLOW", -6: "IO", -7: "FORMAT", -8: "NODEVICE", -9: "NONCANON"}
E_NONCANON = -9


class MfxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("merfin_amd error %s (%d): %s" % (MFX_ERRORS.get(code, "?"), code, msg))
        self.code = code


def lib_path():
    # MFX_LIB: another build of the same sources (kernel A/B experiments: tools/ab_build.sh); never a different ABI
    return os.environ.get("MFX_LIB") or os.path.join(_HERE, "libmerfin_amd.so")


class _KP(C.Structure):
    _fields_ = [("peak", C.c_double), ("n_prob", C.c_uint32),
                ("probK", C.POINTER(C.c_uint32)), ("probP", C.POINTER(C.c_double))]


class _Info(C.Structure):
    _fields_ = [("k", C.c_int), ("canonical", C.c_int), ("capacity", C.c_uint64),
                ("distinct", C.c_uint64), ("bytes", C.c_uint64), ("seq_only", C.c_int), ("compact", C.c_int),
                ("dropped", C.c_uint64)]


class _DbInfo(C.Structure):
    _fields_ = [("k", C.c_int), ("format", C.c_int), ("n_kmers", C.c_uint64), ("placed", C.c_int)]


class _VarOpts(C.Structure):
    _fields_ = [("mode", C.c_int), ("comb", C.c_uint32), ("nosplit", C.c_int), ("debug_path", C.c_char_p)]


INDEX_HEADER_BYTES = 128          # MFX_INDEX_HEADER_BYTES

VARIANT_MODES = {"filter": 4, "polish": 5, "better": 6, "strict": 7, "loose": 8}


class _ReadsStats(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("bases", C.c_uint64), ("kmers", C.c_uint64), ("counted", C.c_uint64),
                ("dropped", C.c_uint64), ("saturated", C.c_uint64), ("seconds_kernel", C.c_double), ("seconds_copy", C.c_double)]


class _SpectrumPeak(C.Structure):
    _fields_ = [("valley", C.c_uint32), ("main_peak", C.c_uint32), ("haploid_peak", C.c_uint32), ("count_at_peak", C.c_uint64)]


class _HistResult(C.Structure):
    _fields_ = [("kasm", C.c_uint64), ("kmissing", C.c_uint64), ("koverCpy", C.c_double),
                ("undrMax", C.c_uint32), ("overMax", C.c_uint32),
                ("undr", C.POINTER(C.c_uint64)), ("over", C.POINTER(C.c_uint64)),
                ("ncontigs", C.c_uint32),
                ("contig_kasm", C.POINTER(C.c_uint64)), ("contig_kmissing", C.POINTER(C.c_uint64))]


_lib = None

# every symbol include/merfin_amd.h declares (tests check the .so exports all of them)
SYMBOLS = [
    "mfx_last_error", "mfx_last_error_code", "mfx_version", "mfx_device_count", "mfx_device_warm", "mfx_device_memory",
    "mfx_index_create", "mfx_index_free", "mfx_index_estimate_gb", "mfx_index_add_read", "mfx_index_add_asm",
    "mfx_index_count_asm", "mfx_index_build_for_hist", "mfx_index_count_claimed", "mfx_hist_run_parts", "mfx_index_create_for_seq", "mfx_index_create_for_seq_lf", "mfx_index_create_lf", "mfx_db_stage_begin", "mfx_index_build_for_hist_staged", "mfx_index_load_db_staged", "mfx_db_stage_free", "mfx_db_stage_boost", "mfx_index_estimate_gb_for_seq", "mfx_index_claim_seq", "mfx_index_value", "mfx_index_get_info", "mfx_index_export",
    "mfx_db_probe", "mfx_index_load_db", "mfx_index_load_db_multi", "mfx_db_write_flat", "mfx_db_convert", "mfx_db_merge", "mfx_db_merge_plan", "mfx_db_join_completeness", "mfx_db_join_spectrum", "mfx_db_join_grain", "mfx_db_join_host", "mfx_db_convert_placed", "mfx_db_write_flat_placed", "mfx_db_place_keys", "mfx_index_save", "mfx_index_load",
    "mfx_index_set_fingerprint", "mfx_index_get_origin",
    "mfx_host_alloc", "mfx_host_free", "mfx_seq_create", "mfx_hist_run_streamed",
    "mfx_hist_run_streamed_multi", "mfx_hist_run_streamed_range", "mfx_hist_stream_share",
    "mfx_index_replicate", "mfx_seq_replicate", "mfx_hist_run_multi", "mfx_hist_run_sharded",
    "mfx_comm_unique_id", "mfx_comm_create", "mfx_comm_free", "mfx_comm_rank", "mfx_comm_size", "mfx_comm_barrier", "mfx_comm_exchange_counts", "mfx_comm_alltoallv",
    "mfx_index_replicate_many", "mfx_seq_replicate_many", "mfx_seq_pack",
    "mfx_hist_allreduce", "mfx_hist_allgather_overflow", "mfx_hist_result_add_overflow",
    "mfx_index_image_header", "mfx_index_create_from_header", "mfx_index_device_image", "mfx_index_commit",
    "mfx_seq_upload", "mfx_seq_from_device", "mfx_seq_free", "mfx_seq_num_contigs", "mfx_seq_num_bases",
    "mfx_seq_num_tiles", "mfx_seq_is_packed",
    "mfx_diag_gather_rate",
    "mfx_eval_create", "mfx_eval_free", "mfx_eval_nbins", "mfx_eval_debug_enable", "mfx_eval_debug_counters", "mfx_eval_debug_worklist", "mfx_eval_debug_worklist_read", "mfx_getK", "mfx_getKmetric", "mfx_histoQV",
    "mfx_hist_run", "mfx_hist_result_free", "mfx_hist_launch", "mfx_hist_launch_cyclic", "mfx_hist_result_from_counts",
    "mfx_hist_take_overflow", "mfx_hist_report", "mfx_diag_stream_rates",
    "mfx_pack_bases", "mfx_host_threads_share", "mfx_dump_values", "mfx_dump_contig", "mfx_dump_values_sharded", "mfx_dump_contig_sharded", "mfx_variants_run_sharded", "mfx_vcf_load", "mfx_vcf_free", "mfx_variants_run_vcf", "mfx_vcf_prepare", "mfx_vcf_path_bound", "mfx_index_claim_paths", "mfx_vcf_prepare_path_index", "mfx_completeness", "mfx_completeness_pieces", "mfx_variants_run",
    "mfx_index_set_shard", "mfx_router_create", "mfx_router_free", "mfx_route_tiles", "mfx_hist_keys_launch",
    "mfx_reads_begin", "mfx_reads_set_filter", "mfx_reads_add", "mfx_reads_end",
    "mfx_reads_begin_all", "mfx_index_growths", "mfx_index_write_db",
    "mfx_reads_begin_range", "mfx_index_key_bins", "mfx_db_writer_open", "mfx_db_writer_append_index", "mfx_db_writer_close", "mfx_db_writer_abort",
    "mfx_db_writer_open_streamed", "mfx_db_writer_append_sorted", "mfx_db_writer_info", "mfx_index_write_db_streamed",
    "mfx_reads_store_create", "mfx_reads_store_add", "mfx_reads_store_info", "mfx_reads_replay", "mfx_reads_store_free",
    "mfx_track_num_windows", "mfx_track_run", "mfx_track_write",
    "mfx_regions_run", "mfx_regions_count", "mfx_regions_tiles_revisited", "mfx_diag_regions_times", "mfx_regions_copy", "mfx_regions_free",
    "mfx_regions_write", "mfx_regions_from_planes_host",
    "mfx_db_merge_except", "mfx_phase_run", "mfx_phase_count", "mfx_phase_copy", "mfx_phase_contig_counts", "mfx_phase_free", "mfx_diag_phase_times", "mfx_phase_write",
    "mfx_phase_from_planes_host",
    "mfx_bin_begin", "mfx_bin_add", "mfx_bin_flush", "mfx_bin_ready", "mfx_bin_take", "mfx_bin_end", "mfx_bin_classify", "mfx_bin_plan_host",
    "mfx_spectrum_run", "mfx_spectrum_peak", "mfx_spectrum_write", "mfx_diag_spectrum_time",
    "mfx_db_trio", "mfx_db_trio_hist", "mfx_db_histogram", "mfx_db_histogram_write", "mfx_db_trio_host",
    "mfx_db_diploid", "mfx_db_diploid_host", "mfx_diploid_write_asm",
    "mfx_debug_traverse_host", "mfx_debug_score_paths", "mfx_debug_score_paths_trv",
]

# the cluster tables of the variant modes' device traverse (csrc/mfx_traverse.h; static_asserted in csrc/mfx_debug.cpp)
TRV_CLUSTER_DTYPE = np.dtype([("win_off", "<u8"), ("win_len", "<u4"), ("nv", "<u4"), ("var0", "<u4"), ("path_cap", "<u4"),
                              ("text0", "<u8"), ("path0", "<u8"), ("row0", "<u8"), ("text_cap", "<u4"), ("pad", "<u4")])
TRV_VARIANT_DTYPE = np.dtype([("off", "<u4"), ("reflen", "<u4"), ("na", "<u4"), ("al0", "<u4")])
TRV_ALLELE_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("pad", "<u4")])
assert (TRV_CLUSTER_DTYPE.itemsize, TRV_VARIANT_DTYPE.itemsize, TRV_ALLELE_DTYPE.itemsize) == (56, 16, 16)
TRV_OK, TRV_RANGE, TRV_ROOM = 0, 1, 2
TRV_MAX_NV, TRV_MAX_PATHS, TRV_MAX_LEN = 8, 64, 640

# one entry of the -hist worklist as Evaluator.debug_worklist_read returns it (include/merfin_amd.h): w = slot | mode << 29 | dbl << 31
WORKLIST_DTYPE = np.dtype([("kmer", "<u8"), ("aux", "<u4"), ("w", "<u4")])
assert WORKLIST_DTYPE.itemsize == 16

# one window of Evaluator.track: the layout of mfx_track_window (include/merfin_amd.h), 72 bytes
TRACK_DTYPE = np.dtype([("n_kmers", "<u4"), ("n_missing", "<u4"), ("n_scored", "<u4"), ("n_pos", "<u4"), ("n_neg", "<u4"),
                        ("n_nonfinite", "<u4"), ("sum_readK", "<u8"), ("sum_asmK", "<u8"), ("sum_kstar_lo", "<u8"),
                        ("sum_kstar_hi", "<i8"), ("min_kstar", "<f8"), ("max_kstar", "<f8")])
assert TRACK_DTYPE.itemsize == 72

# one record of Evaluator.regions: the layout of mfx_region (include/merfin_amd.h), 56 bytes; cls: REGION_CLASSES[cls]
REGION_DTYPE = np.dtype([("contig", "<u4"), ("cls", "<u4"), ("start", "<u8"), ("end", "<u8"), ("n_kmers", "<u8"), ("sum_readK", "<u8"),
                         ("sum_asmK", "<u8"), ("ext_kstar", "<f8")])
assert REGION_DTYPE.itemsize == 56
REGION_CLASSES = ("missing", "collapsed", "expanded")


class _RegionsOpts(C.Structure):
    _fields_ = [("kstar", C.c_double), ("gap", C.c_uint64), ("min_kmers", C.c_uint64)]


# one block of Evaluator.phase: the layout of mfx_phase_block (include/merfin_amd.h), 48 bytes; hap: 0 = A (the read side), 1 = B
PHASE_DTYPE = np.dtype([("contig", "<u4"), ("hap", "<u4"), ("start", "<u8"), ("end", "<u8"), ("n_hap", "<u8"), ("n_switch", "<u8"),
                        ("n_switch_runs", "<u8")])
assert PHASE_DTYPE.itemsize == 48


class _PhaseOpts(C.Structure):
    _fields_ = [("switches", C.c_uint64), ("range", C.c_uint64)]


# the counts of one read of Evaluator.bin_reads: mfx_bin_record (include/merfin_amd.h) is four uint32 -- k-mers, A only, B only, shared
BIN_CLASSES = ("A", "B", "U")


class _BinStats(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("bases", C.c_uint64), ("kmers", C.c_uint64), ("a", C.c_uint64), ("b", C.c_uint64),
                ("shared", C.c_uint64), ("seconds_kernel", C.c_double), ("seconds_copy", C.c_double)]


class _BinOpts(C.Structure):
    _fields_ = [("norm_a", C.c_uint64), ("norm_b", C.c_uint64), ("ratio_milli", C.c_uint32), ("min_hits", C.c_uint32)]


def _share_hip_runtime_with_torch():
    """A process must hold ONE HIP/HSA runtime.  PyTorch-ROCm wheels bundle their
    own libamdhip64.so; if libmerfin_amd.so pulled in /opt/rocm's copy first, a
    later `import torch` would start a second runtime that sees no GPU.  So when
    torch is installed, map its copy first (same SONAME: ours then binds to it)."""
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        p = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(p):
            C.CDLL(p, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def load_library():
    """Load libmerfin_amd.so.  Fails loudly when the HIP library was not built."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise ImportError("merfin_amd: %s is missing -- build it with `make -C merfin_amd/csrc` "
                          "(or __graft_entry__.build()); there is no CPU fallback" % p)
    _share_hip_runtime_with_torch()
    L = C.CDLL(p)
    u64p, u32p, f64p, vp = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.c_void_p
    L.mfx_last_error.restype = C.c_char_p
    L.mfx_version.restype = C.c_char_p
    L.mfx_last_error_code.restype = C.c_int
    L.mfx_device_count.restype = C.c_int
    L.mfx_device_warm.argtypes = [C.c_int]
    L.mfx_device_memory.argtypes = [C.c_int, u64p, u64p]
    L.mfx_index_create.restype = vp
    L.mfx_index_create.argtypes = [C.c_int, C.c_uint64, C.c_double, C.c_int]
    L.mfx_index_free.argtypes = [vp]
    L.mfx_index_estimate_gb.restype = C.c_double
    L.mfx_index_estimate_gb.argtypes = [C.c_int, C.c_uint64]
    L.mfx_index_add_read.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int]
    L.mfx_index_add_asm.argtypes = [vp, vp, vp, C.c_uint64, C.c_int]
    L.mfx_index_count_asm.argtypes = [vp, vp, vp]
    L.mfx_index_count_claimed.argtypes = [vp, vp, vp]
    L.mfx_index_build_for_hist.argtypes = [vp, vp, C.c_char_p, C.c_uint64, C.c_uint64]
    L.mfx_hist_run_parts.argtypes = [C.POINTER(vp), C.POINTER(vp), C.POINTER(C.POINTER(C.c_uint32)), C.c_uint32, C.c_uint32, vp]
    L.mfx_index_create_for_seq.restype = vp
    L.mfx_index_create_for_seq.argtypes = [C.c_int, C.c_uint64, C.c_double, C.c_int]
    L.mfx_index_create_lf.restype = vp
    L.mfx_index_create_lf.argtypes = [C.c_int, C.c_uint64, C.c_double, C.c_int, C.c_double]
    L.mfx_index_create_for_seq_lf.restype = vp
    L.mfx_index_create_for_seq_lf.argtypes = [C.c_int, C.c_uint64, C.c_double, C.c_int, C.c_double]
    L.mfx_db_stage_begin.restype = vp
    L.mfx_db_stage_begin.argtypes = [C.c_char_p, C.c_int]
    L.mfx_index_build_for_hist_staged.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint64]
    L.mfx_index_load_db_staged.argtypes = [vp, vp, C.c_int, C.c_uint64, C.c_uint64]
    L.mfx_db_stage_free.restype = None
    L.mfx_db_stage_free.argtypes = [vp]
    L.mfx_db_stage_boost.restype = None
    L.mfx_db_stage_boost.argtypes = [vp]
    L.mfx_index_estimate_gb_for_seq.restype = C.c_double
    L.mfx_index_estimate_gb_for_seq.argtypes = [C.c_int, C.c_uint64]
    L.mfx_index_claim_seq.argtypes = [vp, vp, vp]
    L.mfx_index_value.argtypes = [vp, u64p, C.c_uint64, u32p, u32p]
    L.mfx_index_get_info.argtypes = [vp, C.POINTER(_Info)]
    L.mfx_index_export.argtypes = [vp, u64p, u32p, u32p, u64p]
    L.mfx_db_probe.argtypes = [C.c_char_p, C.POINTER(_DbInfo)]
    L.mfx_index_load_db.argtypes = [vp, C.c_char_p, C.c_int, C.c_uint64, C.c_uint64]
    L.mfx_db_write_flat.argtypes = [C.c_char_p, C.c_int, u64p, u32p, C.c_uint64]
    L.mfx_db_convert.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64)]
    L.mfx_db_convert_placed.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64)]
    L.mfx_db_merge.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.c_char_p, C.POINTER(DbMergeOpts), C.POINTER(DbMergeStats)]
    L.mfx_db_merge_except.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_char_p), C.c_uint32, C.c_char_p, C.POINTER(DbMergeOpts), C.POINTER(DbMergeStats),
                                      u64p]
    L.mfx_db_merge_plan.argtypes = [C.POINTER(u64p), u64p, C.c_uint32, C.c_int, C.c_uint64, u64p, C.c_uint64, u64p]
    L.mfx_db_join_completeness.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(DbJoinOpts), f64p, f64p, C.POINTER(DbJoinStats)]
    L.mfx_db_join_spectrum.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(DbJoinOpts), u64p, u64p, C.POINTER(DbJoinStats)]
    L.mfx_db_join_grain.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.mfx_db_join_grain.restype = None
    L.mfx_db_join_host.argtypes = [u64p, C.POINTER(C.c_uint32), C.c_uint64, u64p, C.POINTER(C.c_uint32), C.c_uint64, u64p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                   C.c_uint64, u64p]
    L.mfx_db_trio.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(DbTrioOpts), u64p, C.POINTER(DbTrioStats)]
    L.mfx_db_trio_hist.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, u64p, C.POINTER(DbTrioStats), C.c_int]
    L.mfx_db_histogram.argtypes = [C.c_char_p, C.c_uint32, u64p, u64p, C.c_int]
    L.mfx_db_histogram_write.argtypes = [u64p, C.c_uint32, C.c_char_p]
    L.mfx_db_trio_host.argtypes = [u64p, C.POINTER(C.c_uint32), C.c_uint64, u64p, C.POINTER(C.c_uint32), C.c_uint64, u64p, C.POINTER(C.c_uint32), C.c_uint64, C.c_int,
                                   C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u64p, C.POINTER(C.c_uint32), u64p, u64p, C.POINTER(C.c_uint32), u64p, u64p,
                                   C.POINTER(DbTrioStats)]
    L.mfx_db_diploid.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(DbJoinOpts), u64p, u64p, u64p, C.POINTER(DbDiploidStats), f64p, f64p]
    L.mfx_db_diploid_host.argtypes = [u64p, C.POINTER(C.c_uint32), C.c_uint64, u64p, C.POINTER(C.c_uint32), C.c_uint64, u64p, C.POINTER(C.c_uint32), C.c_uint64, C.c_int,
                                      C.POINTER(DbJoinOpts), u64p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint64, u64p, u64p, u64p, u64p,
                                      C.POINTER(DbDiploidStats), f64p, f64p]
    L.mfx_diploid_write_asm.argtypes = [u64p, C.c_uint32, C.c_char_p]
    L.mfx_db_write_flat_placed.argtypes = [C.c_char_p, C.c_int, u64p, u32p, C.c_uint64]
    L.mfx_db_place_keys.argtypes = [C.c_int, vp, C.c_uint64, vp, C.c_int, C.c_int]
    L.mfx_index_load_db_multi.argtypes = [C.POINTER(vp), C.c_uint32, C.c_char_p, C.c_int, C.c_uint64, C.c_uint64]
    L.mfx_index_save.argtypes = [vp, C.c_char_p]
    L.mfx_index_load.restype = vp
    L.mfx_index_load.argtypes = [C.c_char_p, C.c_double, C.c_int]
    L.mfx_index_image_header.argtypes = [vp, vp]
    L.mfx_index_create_from_header.restype = vp
    L.mfx_index_create_from_header.argtypes = [vp, C.c_double, C.c_int]
    L.mfx_index_device_image.argtypes = [vp, C.POINTER(vp), u64p, C.POINTER(vp), u64p]
    L.mfx_index_commit.argtypes = [vp]
    L.mfx_seq_upload.restype = vp
    L.mfx_seq_upload.argtypes = [C.c_int, C.POINTER(C.c_char_p), u64p, C.c_uint32]
    L.mfx_seq_from_device.restype = vp
    L.mfx_seq_from_device.argtypes = [C.c_int, C.POINTER(vp), u64p, C.c_uint32, vp]
    L.mfx_seq_free.argtypes = [vp]
    L.mfx_seq_num_contigs.restype = C.c_uint32
    L.mfx_seq_num_contigs.argtypes = [vp]
    L.mfx_seq_num_bases.restype = C.c_uint64
    L.mfx_seq_num_bases.argtypes = [vp]
    L.mfx_seq_num_tiles.restype = C.c_uint64
    L.mfx_seq_num_tiles.argtypes = [vp]
    L.mfx_eval_create.restype = vp
    L.mfx_eval_create.argtypes = [vp, C.POINTER(_KP), C.c_uint32]
    L.mfx_eval_free.argtypes = [vp]
    L.mfx_eval_nbins.restype = C.c_uint32
    L.mfx_eval_nbins.argtypes = [vp]
    L.mfx_diag_gather_rate.argtypes = [C.c_int, C.c_uint64, C.POINTER(C.c_double)]
    L.mfx_eval_debug_enable.argtypes = [vp, C.c_int]
    L.mfx_eval_debug_counters.argtypes = [vp, u64p]
    L.mfx_eval_debug_worklist.argtypes = [vp, C.c_int, C.c_uint32]
    L.mfx_eval_debug_worklist_read.argtypes = [vp, C.c_int, u32p, u32p, u64p, C.c_uint64, vp, C.c_uint64, u64p]
    L.mfx_getK.argtypes = [C.POINTER(_KP), C.c_uint32, C.c_uint32, f64p, f64p, f64p]
    L.mfx_getKmetric.restype = C.c_double
    L.mfx_getKmetric.argtypes = [C.c_double, C.c_double]
    L.mfx_histoQV.restype = C.c_double
    L.mfx_histoQV.argtypes = [C.c_double, C.c_double, C.c_int]
    L.mfx_hist_run.argtypes = [vp, vp, C.POINTER(_HistResult)]
    L.mfx_hist_result_free.argtypes = [C.POINTER(_HistResult)]
    L.mfx_hist_launch.argtypes = [vp, vp, C.c_uint64, C.c_uint64, vp, vp, vp]
    L.mfx_hist_launch_cyclic.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.mfx_hist_result_from_counts.argtypes = [C.c_uint32, u64p, C.c_double, C.c_uint32, C.POINTER(_HistResult)]
    L.mfx_hist_take_overflow.argtypes = [vp, u64p, C.c_uint64, u64p]
    L.mfx_diag_stream_rates.argtypes = [C.c_int, vp, C.c_uint64, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mfx_hist_report.argtypes = [C.POINTER(_HistResult), C.c_int, C.c_char_p, C.c_char_p]
    L.mfx_dump_values.argtypes = [vp, vp, C.c_uint32, C.c_uint64, C.c_uint64, u32p, u32p, u64p, u64p]
    L.mfx_dump_contig.argtypes = [vp, vp, C.c_uint32, C.c_char_p, C.c_char_p, C.c_int, u64p, u64p]
    L.mfx_dump_values_sharded.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, u32p, u32p, u64p, u64p]
    L.mfx_dump_contig_sharded.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_char_p, C.c_char_p, C.c_int, u64p, u64p]
    L.mfx_variants_run_sharded.argtypes = [vp, C.c_uint32, C.c_char_p, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), u64p, C.c_uint32,
                                           C.POINTER(_VarOpts), C.c_char_p, C.c_char_p, u64p]
    L.mfx_completeness.argtypes = [vp, f64p, f64p]
    L.mfx_completeness_pieces.argtypes = [vp, f64p, f64p]
    L.mfx_index_set_shard.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.mfx_router_create.restype = vp
    L.mfx_router_create.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.mfx_router_free.argtypes = [vp]
    L.mfx_route_tiles.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint32, vp, vp, vp, u64p, vp]
    L.mfx_hist_keys_launch.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp]
    L.mfx_variants_run.argtypes = [vp, C.c_char_p, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), u64p, C.c_uint32,
                                   C.POINTER(_VarOpts), C.c_char_p, C.c_char_p, u64p]
    L.mfx_vcf_load.restype = vp
    L.mfx_vcf_load.argtypes = [C.c_char_p]
    L.mfx_vcf_free.restype = None
    L.mfx_vcf_free.argtypes = [vp]
    L.mfx_variants_run_vcf.argtypes = [vp, vp, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), u64p, C.c_uint32,
                                       C.POINTER(_VarOpts), C.c_char_p, C.c_char_p, u64p]
    L.mfx_vcf_prepare.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), u64p, C.c_uint32, C.POINTER(_VarOpts)]
    L.mfx_vcf_path_bound.argtypes = [vp, u64p]
    L.mfx_index_claim_paths.argtypes = [vp, vp, u64p]
    L.mfx_vcf_prepare_path_index.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), u64p, C.c_uint32, C.POINTER(_VarOpts), C.c_double, C.c_int, C.c_double,
                                             C.POINTER(vp)]
    L.mfx_index_set_fingerprint.argtypes = [vp, C.c_uint64]
    L.mfx_index_get_origin.argtypes = [vp, u64p, u64p, u64p]
    L.mfx_host_threads_share.restype = None
    L.mfx_host_threads_share.argtypes = [C.c_uint]
    L.mfx_pack_bases.restype = None
    L.mfx_pack_bases.argtypes = [vp, C.c_uint64, vp, vp]
    L.mfx_host_alloc.restype = vp
    L.mfx_host_alloc.argtypes = [C.c_size_t]
    L.mfx_host_free.restype = None
    L.mfx_host_free.argtypes = [vp]
    L.mfx_seq_create.restype = vp
    L.mfx_seq_create.argtypes = [C.c_int, u64p, C.c_uint32]
    L.mfx_hist_run_streamed.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(_HistResult)]
    L.mfx_index_replicate.restype = vp
    L.mfx_index_replicate.argtypes = [vp, C.c_int]
    L.mfx_seq_replicate.restype = vp
    L.mfx_seq_replicate.argtypes = [vp, C.c_int]
    L.mfx_hist_run_multi.argtypes = [C.POINTER(vp), C.POINTER(vp), C.c_uint32, C.POINTER(_HistResult)]
    L.mfx_hist_run_streamed_multi.argtypes = [C.POINTER(vp), C.POINTER(vp), C.c_uint32, C.POINTER(vp), C.POINTER(_HistResult)]
    L.mfx_hist_run_streamed_range.argtypes = [vp, vp, C.POINTER(vp), C.c_uint64, C.c_uint64, vp, vp]
    L.mfx_hist_stream_share.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.mfx_hist_run_sharded.argtypes = [C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.c_uint32, C.POINTER(_HistResult)]
    L.mfx_comm_unique_id.argtypes = [vp]
    L.mfx_comm_create.restype = vp
    L.mfx_comm_create.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.mfx_comm_free.restype = None
    L.mfx_comm_free.argtypes = [vp]
    L.mfx_comm_rank.argtypes = [vp]
    L.mfx_comm_size.argtypes = [vp]
    L.mfx_comm_barrier.argtypes = [vp, vp]
    L.mfx_comm_exchange_counts.argtypes = [vp, u64p, u64p, vp]
    L.mfx_comm_alltoallv.argtypes = [vp, vp, u64p, vp, u64p, C.c_uint32, vp]
    L.mfx_index_replicate_many.argtypes = [vp, C.POINTER(C.c_int), C.c_uint32, C.POINTER(vp)]
    L.mfx_seq_replicate_many.argtypes = [vp, C.POINTER(C.c_int), C.c_uint32, C.POINTER(vp)]
    L.mfx_seq_pack.argtypes = [vp]
    L.mfx_hist_allreduce.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, vp]
    L.mfx_hist_allgather_overflow.argtypes = [vp, vp, u64p, C.c_uint64, u64p, vp]
    L.mfx_hist_result_add_overflow.argtypes = [C.POINTER(_HistResult), u64p, C.c_uint64]
    L.mfx_reads_begin.restype = vp
    L.mfx_reads_begin.argtypes = [vp, C.c_uint64]
    L.mfx_reads_set_filter.argtypes = [vp, C.c_uint64, C.c_uint64]
    L.mfx_reads_add.argtypes = [vp, C.POINTER(C.c_char_p), u64p, C.c_uint64]
    L.mfx_reads_end.argtypes = [vp, C.POINTER(_ReadsStats)]
    L.mfx_reads_begin_all.restype = vp
    L.mfx_reads_begin_all.argtypes = [vp, C.c_uint64]
    L.mfx_index_growths.argtypes = [vp, u64p, C.POINTER(C.c_double), C.POINTER(C.c_double), u64p]
    L.mfx_index_write_db.argtypes = [vp, C.c_int, C.c_char_p, u64p]
    L.mfx_reads_begin_range.restype = vp
    L.mfx_reads_begin_range.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64]
    L.mfx_index_key_bins.argtypes = [vp, C.c_int, u64p, C.POINTER(C.c_uint32)]
    L.mfx_db_writer_open.restype = vp
    L.mfx_db_writer_open.argtypes = [C.c_char_p, C.c_int]
    L.mfx_db_writer_append_index.argtypes = [vp, vp, C.c_int, u64p]
    L.mfx_db_writer_close.argtypes = [vp, u64p]
    L.mfx_db_writer_abort.restype = None
    L.mfx_db_writer_abort.argtypes = [vp]
    L.mfx_db_writer_open_streamed.restype = vp
    L.mfx_db_writer_open_streamed.argtypes = [C.c_char_p, C.c_int]
    L.mfx_db_writer_append_sorted.argtypes = [vp, u64p, C.POINTER(C.c_uint32), C.c_uint64]
    L.mfx_db_writer_info.argtypes = [vp, u64p, u64p, u64p, u64p, u64p]
    L.mfx_index_write_db_streamed.argtypes = [vp, C.c_int, C.c_char_p, u64p]
    L.mfx_reads_store_create.restype = vp
    L.mfx_reads_store_create.argtypes = [C.c_int, C.c_uint64, C.c_uint64]
    L.mfx_reads_store_add.argtypes = [vp, C.POINTER(C.c_char_p), u64p, C.c_uint64]
    L.mfx_reads_store_info.argtypes = [vp, u64p, u64p, u64p, u64p, C.POINTER(C.c_int)]
    L.mfx_reads_replay.argtypes = [vp, vp, C.c_uint64, C.c_uint64]
    L.mfx_reads_store_free.restype = None
    L.mfx_reads_store_free.argtypes = [vp]
    L.mfx_track_num_windows.restype = C.c_uint64
    L.mfx_track_num_windows.argtypes = [vp, C.c_uint64]
    L.mfx_track_run.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, u64p, u64p, u64p]
    L.mfx_track_write.argtypes = [vp, C.c_uint64, vp, C.POINTER(C.c_char_p), C.c_uint64, C.c_char_p, C.c_char_p]
    L.mfx_regions_run.argtypes = [vp, vp, C.POINTER(_RegionsOpts), C.POINTER(vp), u64p, u64p]
    L.mfx_regions_count.restype = C.c_uint64
    L.mfx_regions_count.argtypes = [vp]
    L.mfx_regions_tiles_revisited.restype = C.c_uint64
    L.mfx_regions_tiles_revisited.argtypes = [vp]
    L.mfx_diag_regions_times.restype = None
    L.mfx_diag_regions_times.argtypes = [vp, C.POINTER(C.c_double)]
    L.mfx_regions_copy.argtypes = [vp, vp, C.c_uint64]
    L.mfx_regions_free.restype = None
    L.mfx_regions_free.argtypes = [vp]
    L.mfx_regions_write.argtypes = [vp, C.c_uint64, vp, C.POINTER(C.c_char_p), C.c_int, C.c_char_p]
    L.mfx_regions_from_planes_host.argtypes = [vp, u64p, C.c_uint32, C.POINTER(_RegionsOpts), vp, C.c_uint64, u64p]
    L.mfx_phase_run.argtypes = [vp, vp, C.POINTER(_PhaseOpts), C.POINTER(vp)]
    L.mfx_phase_count.restype = C.c_uint64
    L.mfx_phase_count.argtypes = [vp]
    L.mfx_phase_copy.argtypes = [vp, vp, C.c_uint64]
    L.mfx_phase_contig_counts.argtypes = [vp, vp, C.c_uint64]
    L.mfx_phase_free.restype = None
    L.mfx_phase_free.argtypes = [vp]
    L.mfx_diag_phase_times.restype = None
    L.mfx_diag_phase_times.argtypes = [vp, C.POINTER(C.c_double)]
    L.mfx_phase_write.argtypes = [vp, C.c_uint64, vp, vp, C.POINTER(C.c_char_p), C.c_int, C.POINTER(_PhaseOpts), C.c_char_p]
    L.mfx_phase_from_planes_host.argtypes = [vp, u64p, C.c_uint32, C.c_int, C.POINTER(_PhaseOpts), vp, C.c_uint64, u64p]
    L.mfx_bin_begin.restype = vp
    L.mfx_bin_begin.argtypes = [vp, C.c_uint64]
    L.mfx_bin_add.argtypes = [vp, C.POINTER(C.c_char_p), u64p, C.c_uint64]
    L.mfx_bin_flush.argtypes = [vp]
    L.mfx_bin_ready.restype = C.c_uint64
    L.mfx_bin_ready.argtypes = [vp]
    L.mfx_bin_take.argtypes = [vp, vp, C.c_uint64, u64p]
    L.mfx_bin_end.argtypes = [vp, C.POINTER(_BinStats)]
    L.mfx_bin_classify.argtypes = [vp, C.c_uint64, C.POINTER(_BinOpts), vp]
    L.mfx_bin_plan_host.argtypes = [u64p, C.c_uint64, C.c_int, C.c_uint64, vp, C.c_uint64, u64p]
    L.mfx_spectrum_run.argtypes = [vp, C.c_uint32, C.c_uint32, u64p, u64p]
    L.mfx_diag_spectrum_time.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(C.c_float)]
    L.mfx_spectrum_peak.argtypes = [u64p, C.c_uint32, C.POINTER(_SpectrumPeak)]
    L.mfx_spectrum_write.argtypes = [u64p, C.c_uint32, C.c_uint32, C.c_int, C.c_char_p]
    u64 = C.c_uint64
    tables = [vp, u64, vp, u64, vp, u64, vp, u64, vp, u64, u64, u64, u64]       # clusters .. al_bytes, text_end, path_cap, row_cap
    paths = [vp, u64, u64, u64, vp, vp, vp, vp, vp, vp, vp, vp]                # text, len, npaths, nvals, off .. vlen
    L.mfx_debug_traverse_host.argtypes = tables + [vp] * 11
    L.mfx_debug_score_paths.argtypes = [vp] + paths + [C.c_int, vp, vp]
    L.mfx_debug_score_paths_trv.argtypes = [vp] + paths + tables + [C.c_int] + [vp] * 13
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise MfxError(rc, load_library().mfx_last_error().decode())


def _need(ptr):
    if not ptr:
        L = load_library()
        raise MfxError(L.mfx_last_error_code() or -3, L.mfx_last_error().decode())
    return ptr


def device_count():
    return load_library().mfx_device_count()


def device_warm(device=0):
    """context, code object and pinned-memory path of the device brought up now (mfx_device_warm)"""
    _check(load_library().mfx_device_warm(device))


def device_memory(device=0):
    """(free, total) bytes of the device's memory (mfx_device_memory)"""
    f, t = C.c_uint64(0), C.c_uint64(0)
    _check(load_library().mfx_device_memory(device, C.byref(f), C.byref(t)))
    return f.value, t.value


def hist_words(nbins, ncontigs):
    return 2 * nbins + 3 + 2 * ncontigs


class KParams:
    """-peak and the -prob table (merfin-globals.H:226-227,239)."""

    def __init__(self, peak, probK=None, probP=None):
        self.peak = float(peak)
        self.probK = np.ascontiguousarray(probK if probK is not None else [], dtype=np.uint32)
        self.probP = np.ascontiguousarray(probP if probP is not None else [], dtype=np.float64)
        assert len(self.probK) == len(self.probP)
        self.c = _KP(self.peak, len(self.probK),
                     self.probK.ctypes.data_as(C.POINTER(C.c_uint32)), self.probP.ctypes.data_as(C.POINTER(C.c_double)))

    @staticmethod
    def from_file(peak, path):
        """load_Kmetric (merfin-globals.C:21-62): lines with exactly two comma-separated fields."""
        K, P = [], []
        with open(path) as f:
            for line in f:
                w = [x for x in line.rstrip("\r\n").split(",") if x != ""]
                if len(w) == 2:
                    K.append(int(w[0]))
                    P.append(float(w[1]))
        return KParams(peak, K, P)


def getK(kp, readV, asmV):
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    load_library().mfx_getK(C.byref(kp.c), readV, asmV, C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def getKmetric(readK, asmK):
    return load_library().mfx_getKmetric(readK, asmK)


def histoQV(kval, ktot, k):
    return load_library().mfx_histoQV(kval, ktot, k)


def db_probe(path):
    """merylFileReader(path): (k, format, n_kmers) of a k-mer database on disk"""
    i = _DbInfo()
    _check(load_library().mfx_db_probe(path.encode(), C.byref(i)))
    d = {"k": i.k, "format": {1: "meryl", 2: "text", 3: "flat"}.get(i.format), "n_kmers": i.n_kmers}
    if i.placed:
        d["placed"] = True                                      # (only a placed flat file says so: mfx_db_convert_placed)
    return d


def load_db_multi(indexes, path, side, minV=0, maxV=2**64 - 1):
    """one pass over a k-mer database into several tables (the shards of one process)"""
    n = len(indexes)
    arr = (C.c_void_p * n)(*[ix.h for ix in indexes])
    _check(load_library().mfx_index_load_db_multi(arr, n, path.encode(), side, minV, maxV))


def db_convert(in_path, out_path):
    """any accepted database -> the flat form (sorted: delta-coded blocks); returns the number of k-mers (mfx_db_convert, host only)"""
    n = C.c_uint64(0)
    _check(load_library().mfx_db_convert(in_path.encode(), out_path.encode(), C.byref(n)))
    return n.value


MERGE_OPS = {"sum": 0, "max": 1, "min": 2, "intersect": 3}       # MFX_MERGE_*


class DbMergeOpts(C.Structure):
    _fields_ = [("op", C.c_int), ("minV", C.c_uint64), ("maxV", C.c_uint64), ("device", C.c_int)]


class DbMergeStats(C.Structure):
    _fields_ = [("n_in", C.c_uint64), ("n_out", C.c_uint64), ("n_filtered", C.c_uint64), ("n_saturated", C.c_uint64), ("windows", C.c_uint64)]


def db_merge(paths, out_path, op="sum", min_count=0, max_count=2**32 - 1, device=0):
    """sorted flat databases combined on the GPU, window by window (mfx_db_merge): op "sum", "max", "min" (unions) or "intersect" (or a
    number, passed on as it is); a k-mer is written iff min_count <= combined count <= max_count.  One path: a filter.  The file is what
    db_write_flat makes of the result.  Returns the stats: n_in, n_out, n_filtered, n_saturated, windows."""
    paths = [paths] if isinstance(paths, (str, bytes)) else list(paths)
    arr = (C.c_char_p * max(1, len(paths)))(*[p.encode() if isinstance(p, str) else p for p in paths])
    o = DbMergeOpts(MERGE_OPS[op] if isinstance(op, str) else int(op), int(min_count), int(max_count), int(device))
    st = DbMergeStats()
    _check(load_library().mfx_db_merge(arr, len(paths), out_path.encode(), C.byref(o), C.byref(st)))
    return {name: int(getattr(st, name)) for name, _ in DbMergeStats._fields_}


def db_merge_except(paths, not_paths, out_path, op="sum", min_count=0, max_count=2**32 - 1, device=0):
    """db_merge over `paths` without the k-mers that a database of `not_paths` holds, whatever its count there (mfx_db_merge_except: set
    difference); the count written is the operation's over `paths` alone, the filter acts on it.  No not_paths: db_merge, byte for byte.
    Returns db_merge's stats and n_subtracted: the k-mers the operation yields and a database of not_paths holds."""
    paths = [paths] if isinstance(paths, (str, bytes)) else list(paths)
    not_paths = [not_paths] if isinstance(not_paths, (str, bytes)) else list(not_paths)
    enc = lambda ps: (C.c_char_p * max(1, len(ps)))(*[p.encode() if isinstance(p, str) else p for p in ps])
    o = DbMergeOpts(MERGE_OPS[op] if isinstance(op, str) else int(op), int(min_count), int(max_count), int(device))
    st = DbMergeStats()
    sub = C.c_uint64(0)
    _check(load_library().mfx_db_merge_except(enc(paths), len(paths), enc(not_paths), len(not_paths), out_path.encode(), C.byref(o), C.byref(st), C.byref(sub)))
    out = {name: int(getattr(st, name)) for name, _ in DbMergeStats._fields_}
    out["n_subtracted"] = sub.value
    return out


class DbJoinOpts(C.Structure):
    _fields_ = [("device", C.c_int), ("minV", C.c_uint64), ("maxV", C.c_uint64), ("peak", C.c_double), ("n_prob", C.c_uint32), ("probK", C.POINTER(C.c_uint32)),
                ("probP", C.POINTER(C.c_double)), ("copies", C.c_uint32), ("max_mult", C.c_uint32)]


class DbJoinStats(C.Structure):
    _fields_ = [("n_read", C.c_uint64), ("n_asm", C.c_uint64), ("n_both", C.c_uint64), ("windows", C.c_uint64), ("t_read", C.c_double), ("t_decode", C.c_double),
                ("t_join", C.c_double), ("t_total", C.c_double)]


def _join_stats(st):
    return {name: (float if name.startswith("t_") else int)(getattr(st, name)) for name, _ in DbJoinStats._fields_}


def db_join_completeness(read_path, asm_path, kparams, device=0, with_stats=False, min_count=0, max_count=2**32 - 1):
    """-completeness of two sorted flat databases without a table (mfx_db_join_completeness): (total[64], undrcpy[64]) per piece, the
    doubles Evaluator.completeness_pieces gives for a full index of the two files; with_stats: also n_read, n_asm, n_both, windows and
    the call's time split.  min_count / max_count are passed on and take no part: -completeness uses the raw read count"""
    kp = kparams if isinstance(kparams, KParams) else KParams(kparams)
    o = DbJoinOpts(int(device), int(min_count), int(max_count), kp.peak, len(kp.probK), kp.probK.ctypes.data_as(C.POINTER(C.c_uint32)), kp.probP.ctypes.data_as(C.POINTER(C.c_double)), 0, 0)
    t = np.zeros(64, dtype=np.float64)
    u = np.zeros(64, dtype=np.float64)
    st = DbJoinStats()
    _check(load_library().mfx_db_join_completeness(read_path.encode(), asm_path.encode(), C.byref(o), t.ctypes.data_as(C.POINTER(C.c_double)),
                                                   u.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st)))
    return (t, u, _join_stats(st)) if with_stats else (t, u)


def db_join_spectrum(read_path, asm_path, copies=4, max_mult=10000, min_count=0, max_count=2**32 - 1, device=0, with_entries=False, with_stats=False):
    """the copy-number spectrum of two sorted flat databases without a table (mfx_db_join_spectrum): the (copies + 2, max_mult + 1) uint64
    array Index.spectrum gives for a full index of the two files, the read counts through min_count / max_count; with_entries: also the
    number of counted entries; with_stats: also the stats"""
    o = DbJoinOpts(int(device), int(min_count), int(max_count), 0.0, 0, None, None, int(copies), int(max_mult))
    img = np.zeros((max(int(copies), 0) + 2, max(int(max_mult), 0) + 1), dtype=np.uint64)
    n = C.c_uint64(0)
    st = DbJoinStats()
    _check(load_library().mfx_db_join_spectrum(read_path.encode(), asm_path.encode(), C.byref(o), img.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n), C.byref(st)))
    out = (img,) + ((n.value,) if with_entries else ()) + ((_join_stats(st),) if with_stats else ())
    return out if len(out) > 1 else img


def db_join_grain():
    """(merged positions per lane, per workgroup tile) of the join kernel (csrc/mfx_join.h)"""
    per, tile = C.c_uint32(0), C.c_uint32(0)
    load_library().mfx_db_join_grain(C.byref(per), C.byref(tile))
    return per.value, tile.value


def db_join_host(read_keys, read_vals, asm_keys, asm_vals):
    """the join kernel's walk on the host (mfx_db_join_host): (k-mers, read counts, asm counts), one per distinct k-mer, in the order the
    lanes meet them"""
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    rk = np.ascontiguousarray(read_keys, dtype=np.uint64)
    rv = np.ascontiguousarray(read_vals, dtype=np.uint32)
    ak = np.ascontiguousarray(asm_keys, dtype=np.uint64)
    av = np.ascontiguousarray(asm_vals, dtype=np.uint32)
    cap = len(rk) + len(ak)
    keys = np.zeros(max(cap, 1), dtype=np.uint64)
    orv = np.zeros(max(cap, 1), dtype=np.uint32)
    oav = np.zeros(max(cap, 1), dtype=np.uint32)
    n = C.c_uint64(0)
    _check(load_library().mfx_db_join_host(rk.ctypes.data_as(u64p), rv.ctypes.data_as(u32p), len(rk), ak.ctypes.data_as(u64p), av.ctypes.data_as(u32p), len(ak),
                                           keys.ctypes.data_as(u64p), orv.ctypes.data_as(u32p), oav.ctypes.data_as(u32p), cap, C.byref(n)))
    assert n.value <= cap
    return keys[:n.value], orv[:n.value], oav[:n.value]


class DiploidCounts(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("distinct", "total", "only_distinct", "only_total", "found")]


class DbDiploidStats(C.Structure):
    _fields_ = [(n, DiploidCounts) for n in ("hap1", "hap2", "both")] + [(n, C.c_uint64) for n in ("solid", "n_read", "n_hap1", "n_hap2", "n_shared", "windows")] + \
               [(n, C.c_double) for n in ("t_read", "t_decode", "t_pair", "t_join", "t_total")]


DIPLOID_CLASSES = ("read-only", "hap1-only", "hap2-only", "shared")      # the rows of the class image


def _diploid_stats(st):
    out = {}
    for name, typ in DbDiploidStats._fields_:
        v = getattr(st, name)
        out[name] = {f: int(getattr(v, f)) for f, _ in DiploidCounts._fields_} if typ is DiploidCounts else (float if name.startswith("t_") else int)(v)
    return out


def _diploid_opts(kparams, copies, max_mult, min_count, max_count, device):
    kp = None if kparams is None else kparams if isinstance(kparams, KParams) else KParams(kparams)
    if kp is None:
        return DbJoinOpts(int(device), int(min_count), int(max_count), 0.0, 0, None, None, int(copies), int(max_mult)), None
    return DbJoinOpts(int(device), int(min_count), int(max_count), kp.peak, len(kp.probK), kp.probK.ctypes.data_as(C.POINTER(C.c_uint32)),
                      kp.probP.ctypes.data_as(C.POINTER(C.c_double)), int(copies), int(max_mult)), kp


def _diploid_result(asm_img, cn_img, n, st, t, u):
    out = {"asm_img": asm_img, "cn_img": cn_img, "n_entries": int(n.value), "stats": _diploid_stats(st)}
    if t is not None:
        out["total"], out["undrcpy"] = t, u
    return out


def db_diploid(read_path, hap1_path, hap2_path, copies=4, max_mult=10000, min_count=0, max_count=2**32 - 1, kparams=None, device=0):
    """two haplotype assemblies against the reads in one windowed join of three sorted flat databases (mfx_db_diploid; the rule:
    csrc/mfx_diploid.h).  Returns a dict: asm_img, the (4, max_mult + 1) class image (rows DIPLOID_CLASSES, column the read count through
    min_count / max_count); cn_img, the (copies + 2, max_mult + 1) copy-number image db_join_spectrum gives for the reads and
    db_merge([hap1, hap2]); n_entries; stats (hap1 / hap2 / both: distinct, total, only_distinct, only_total, found; solid, n_read, n_hap1,
    n_hap2, n_shared, windows, the time split); with kparams also total (64) and undrcpy (3, 64), db_join_completeness' sums for hap1,
    hap2 and the merged database.  QV and completeness derived from the counters are unvalidated against Merqury."""
    o, kp = _diploid_opts(kparams, copies, max_mult, min_count, max_count, device)
    u64p, f64p = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    asm_img = np.zeros((4, max(int(max_mult), 0) + 1), dtype=np.uint64)
    cn_img = np.zeros((max(int(copies), 0) + 2, max(int(max_mult), 0) + 1), dtype=np.uint64)
    t = np.zeros(64, dtype=np.float64) if kp is not None else None
    u = np.zeros((3, 64), dtype=np.float64) if kp is not None else None
    n, st = C.c_uint64(0), DbDiploidStats()
    _check(load_library().mfx_db_diploid(_enc(read_path), _enc(hap1_path), _enc(hap2_path), C.byref(o), asm_img.ctypes.data_as(u64p), cn_img.ctypes.data_as(u64p),
                                         C.byref(n), C.byref(st), None if t is None else t.ctypes.data_as(f64p), None if u is None else u.ctypes.data_as(f64p)))
    return _diploid_result(asm_img, cn_img, n, st, t, u)


def db_diploid_host(reads, hap1, hap2, k, copies=4, max_mult=10000, min_count=0, max_count=2**32 - 1, kparams=None):
    """db_diploid on the host (mfx_db_diploid_host: the text the kernels run) over three (k-mers, counts) pairs of strictly ascending arrays
    of k-mers of length k.  Returns db_diploid's dict and "kmers": (k-mers, read counts, hap1 counts, hap2 counts), one per distinct k-mer in
    the order the lanes meet them."""
    o, kp = _diploid_opts(kparams, copies, max_mult, min_count, max_count, 0)
    u64p, u32p, f64p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    arrs, args = [], []
    for pair in (reads, hap1, hap2):
        arrs.append((np.ascontiguousarray(pair[0], dtype=np.uint64), np.ascontiguousarray(pair[1], dtype=np.uint32)))
        args += [arrs[-1][0].ctypes.data_as(u64p), arrs[-1][1].ctypes.data_as(u32p), len(arrs[-1][0])]
    cap = sum(len(a[0]) for a in arrs)
    keys = np.zeros(max(cap, 1), dtype=np.uint64)
    rv, c1, c2 = (np.zeros(max(cap, 1), dtype=np.uint32) for _ in range(3))
    asm_img = np.zeros((4, max(int(max_mult), 0) + 1), dtype=np.uint64)
    cn_img = np.zeros((max(int(copies), 0) + 2, max(int(max_mult), 0) + 1), dtype=np.uint64)
    t = np.zeros(64, dtype=np.float64) if kp is not None else None
    u = np.zeros((3, 64), dtype=np.float64) if kp is not None else None
    nk, n, st = C.c_uint64(0), C.c_uint64(0), DbDiploidStats()
    _check(load_library().mfx_db_diploid_host(*args, int(k), C.byref(o), keys.ctypes.data_as(u64p), rv.ctypes.data_as(u32p), c1.ctypes.data_as(u32p), c2.ctypes.data_as(u32p),
                                              cap, C.byref(nk), asm_img.ctypes.data_as(u64p), cn_img.ctypes.data_as(u64p), C.byref(n), C.byref(st),
                                              None if t is None else t.ctypes.data_as(f64p), None if u is None else u.ctypes.data_as(f64p)))
    assert nk.value <= cap
    out = _diploid_result(asm_img, cn_img, n, st, t, u)
    out["kmers"] = (keys[:nk.value], rv[:nk.value], c1[:nk.value], c2[:nk.value])
    return out


def diploid_write_asm(img, path):
    """the class image as text (mfx_diploid_write_asm; host only): Assembly, kmer_multiplicity, Count per non-zero cell, the rows labelled
    DIPLOID_CLASSES; .gz / .bz2 / .xz names are compressed"""
    img = np.ascontiguousarray(img, dtype=np.uint64)
    if img.ndim != 2 or img.shape[0] != 4:
        raise ValueError("diploid_write_asm: the class image has 4 rows")
    _check(load_library().mfx_diploid_write_asm(img.ctypes.data_as(C.POINTER(C.c_uint64)), img.shape[1] - 1, _enc(path)))


class DbTrioOpts(C.Structure):
    _fields_ = [("cut_mat", C.c_uint32), ("cut_pat", C.c_uint32), ("cut_child", C.c_uint32), ("max_mult", C.c_uint32), ("device", C.c_int)]


class DbTrioStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_mat", "n_pat", "n_child", "n_both", "n_mat_only", "n_pat_only", "n_mat_only_cut", "n_pat_only_cut", "n_child_cut", "n_a",
                                          "n_b", "windows")] + \
               [(n, C.c_uint32) for n in ("cut_mat", "cut_pat", "cut_child", "auto_mat", "auto_pat", "auto_child", "hist_pass", "reserved")] + \
               [(n, C.c_double) for n in ("t_read", "t_decode", "t_merge", "t_hist", "t_classify", "t_write", "t_close", "t_total")]


def _trio_stats(st):
    return {name: (float if name.startswith("t_") else int)(getattr(st, name)) for name, _ in DbTrioStats._fields_ if name != "reserved"}


def _enc(p):
    return None if p is None else p.encode() if isinstance(p, str) else p


def db_trio(mat, pat, child, out_a, out_b, cut_mat=0, cut_pat=0, cut_child=0, max_mult=10000, device=0, with_image=False):
    """the two hap-mer databases of a trio (mfx_db_trio): out_a holds the k-mers of `mat` with a count of cut_mat or more that `pat` does not
    hold -- and, with a child database, that the child holds cut_child times or more, with the smaller of the two counts --, out_b the same
    with the parents swapped.  child None: parents alone.  A cutoff of 0 is read off the valley of its histogram row (spectrum_peak); a row
    without one raises MfxError (E_NODATA).  The rule is this library's own and unvalidated against Merqury.  Returns the stats (k-mers of
    the inputs, of both parents, of one alone, at or above the cutoffs, written to A and B, windows, the cutoffs used and whether each was
    automatic, the time split); with_image: also the (3, max_mult + 1) histogram image, or None when no cutoff was automatic."""
    o = DbTrioOpts(int(cut_mat), int(cut_pat), int(cut_child), int(max_mult), int(device))
    st = DbTrioStats()
    img = np.zeros((3, max(int(max_mult), 0) + 1), dtype=np.uint64)
    _check(load_library().mfx_db_trio(_enc(mat), _enc(pat), _enc(child), _enc(out_a), _enc(out_b), C.byref(o), img.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(st)))
    out = _trio_stats(st)
    return (out, img if st.hist_pass else None) if with_image else out


def db_trio_hist(mat, pat, child=None, max_mult=10000, device=0, with_stats=False):
    """the histogram image of db_trio's first pass (mfx_db_trio_hist): (3, max_mult + 1) uint64 -- row 0 the k-mers `pat` does not hold by
    their count in `mat`, row 1 the k-mers `mat` does not hold by their count in `pat`, row 2 every k-mer of `child` by its count (zeros
    without one); the last column takes the counts of max_mult and more"""
    st = DbTrioStats()
    img = np.zeros((3, max(int(max_mult), 0) + 1), dtype=np.uint64)
    _check(load_library().mfx_db_trio_hist(_enc(mat), _enc(pat), _enc(child), int(max_mult), img.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(st), int(device)))
    return (img, _trio_stats(st)) if with_stats else img


def db_histogram(path, max_mult=10000, device=0, with_count=False):
    """the k-mer histogram of one sorted flat database (mfx_db_histogram; `meryl histogram`): max_mult + 1 uint64 cells, cell m the
    k-mers of count m, the last those of max_mult and more; with_count: also the k-mers of the file"""
    row = np.zeros(max(int(max_mult), 0) + 1, dtype=np.uint64)
    n = C.c_uint64(0)
    _check(load_library().mfx_db_histogram(_enc(path), int(max_mult), row.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n), int(device)))
    return (row, n.value) if with_count else row


def db_histogram_write(row, path):
    """a histogram row as text (mfx_db_histogram_write; host only): count, k-mers per non-zero cell -- the two columns GenomeScope reads;
    .gz / .bz2 / .xz names are compressed.  Unvalidated against `meryl histogram`."""
    row = np.ascontiguousarray(row, dtype=np.uint64)
    _check(load_library().mfx_db_histogram_write(row.ctypes.data_as(C.POINTER(C.c_uint64)), len(row) - 1, _enc(path)))


def db_trio_host(mat, pat, child, cut_mat, cut_pat, cut_child=1, max_mult=10000):
    """db_trio's rule on the host (mfx_db_trio_host; csrc/mfx_trio.h as the kernels run it) over (k-mers, counts) pairs of ascending arrays;
    child None: no child.  Returns ((A k-mers, A counts), (B k-mers, B counts), image, stats)."""
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    has_child = child is not None
    arrs = []
    for pair in (mat, pat, child if has_child else (np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32))):
        arrs.append((np.ascontiguousarray(pair[0], dtype=np.uint64), np.ascontiguousarray(pair[1], dtype=np.uint32)))
    ak, av = np.zeros(max(len(arrs[0][0]), 1), dtype=np.uint64), np.zeros(max(len(arrs[0][0]), 1), dtype=np.uint32)
    bk, bv = np.zeros(max(len(arrs[1][0]), 1), dtype=np.uint64), np.zeros(max(len(arrs[1][0]), 1), dtype=np.uint32)
    img = np.zeros((3, max(int(max_mult), 0) + 1), dtype=np.uint64)
    na, nb, st = C.c_uint64(0), C.c_uint64(0), DbTrioStats()
    args = []
    for k_, v_ in arrs:
        args += [k_.ctypes.data_as(u64p), v_.ctypes.data_as(u32p), len(k_)]
    _check(load_library().mfx_db_trio_host(*args, 1 if has_child else 0, int(cut_mat), int(cut_pat), int(cut_child), int(max_mult), ak.ctypes.data_as(u64p),
                                           av.ctypes.data_as(u32p), C.byref(na), bk.ctypes.data_as(u64p), bv.ctypes.data_as(u32p), C.byref(nb),
                                           img.ctypes.data_as(u64p), C.byref(st)))
    return (ak[:na.value], av[:na.value]), (bk[:nb.value], bv[:nb.value]), img, _trio_stats(st)


def db_merge_plan(firsts, counts, k, R):
    """the key windows mfx_db_merge cuts for inputs whose blocks start at firsts[i] (ascending uint64, ceil(counts[i] / 4096) of them): a list of
    (lo, hi, pairs, [(b0, b1) per input]) (mfx_db_merge_plan, host only)"""
    L = load_library()
    u64p = C.POINTER(C.c_uint64)
    n_in = len(firsts)
    keep = [np.ascontiguousarray(f, dtype=np.uint64) for f in firsts]
    fp = (u64p * max(1, n_in))(*[f.ctypes.data_as(u64p) for f in keep])
    n = np.asarray(counts, dtype=np.uint64)
    nw = C.c_uint64(0)
    _check(L.mfx_db_merge_plan(fp, n.ctypes.data_as(u64p), n_in, k, R, None, 0, C.byref(nw)))
    row = 3 + 2 * n_in
    out = np.zeros(nw.value * row, dtype=np.uint64)
    _check(L.mfx_db_merge_plan(fp, n.ctypes.data_as(u64p), n_in, k, R, out.ctypes.data_as(u64p), nw.value, C.byref(nw)))
    out = out.reshape(-1, row)
    return [(int(r[0]), int(r[1]), int(r[2]), [(int(r[3 + 2 * i]), int(r[4 + 2 * i])) for i in range(n_in)]) for r in out]


def db_convert_placed(in_path, out_path):
    """any accepted canonical database (13 <= k <= 30) -> the PLACED flat form: records sorted by their place in the compact table
    (mfx_db_convert_placed, host only); returns the number of k-mers"""
    n = C.c_uint64(0)
    _check(load_library().mfx_db_convert_placed(in_path.encode(), out_path.encode(), C.byref(n)))
    return n.value


def db_place_keys(k, kmers, out=None, device=0):
    """the placement numbers P (csrc/mfx_place.h) of k-mers: numpy uint64 arrays on the host, or torch int64 CUDA tensors on the device"""
    if isinstance(kmers, np.ndarray):
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        out = np.empty_like(kmers) if out is None else out
        _check(load_library().mfx_db_place_keys(k, C.c_void_p(kmers.ctypes.data), len(kmers), C.c_void_p(out.ctypes.data), 0, device))
        return out
    import torch
    out = torch.empty_like(kmers) if out is None else out
    _check(load_library().mfx_db_place_keys(k, C.c_void_p(kmers.data_ptr()), kmers.numel(), C.c_void_p(out.data_ptr()), 1, device))
    return out


def db_write_flat_placed(path, k, pkeys, values):
    """ascending placement numbers (db_place_keys of the k-mers, sorted) and their counts -> a placed flat file"""
    pkeys = np.ascontiguousarray(pkeys, dtype=np.uint64)
    values = np.ascontiguousarray(values, dtype=np.uint32)
    _check(load_library().mfx_db_write_flat_placed(path.encode(), k, pkeys.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                   values.ctypes.data_as(C.POINTER(C.c_uint32)), len(pkeys)))


def db_write_flat(path, k, kmers, values):
    kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
    values = np.ascontiguousarray(values, dtype=np.uint32)
    _check(load_library().mfx_db_write_flat(path.encode(), k, kmers.ctypes.data_as(C.POINTER(C.c_uint64)),
                                            values.ctypes.data_as(C.POINTER(C.c_uint32)), len(kmers)))


def _ptr(x):
    """host numpy array or device pointer (int / torch tensor) -> (void*, on_device, keepalive)"""
    if isinstance(x, np.ndarray):
        return C.c_void_p(x.ctypes.data), 0, x
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr()), (1 if x.is_cuda else 0), x
    return C.c_void_p(int(x)), 1, None


class DbStage:
    """A delta-coded flat database on its way into device memory (mfx_db_stage_begin); None-like (ok == False) when it cannot be staged."""

    def __init__(self, path, device=0):
        self.h = load_library().mfx_db_stage_begin(path.encode(), device)
        self.ok = bool(self.h)
        self.why = None if self.ok else load_library().mfx_last_error().decode()

    def boost(self):
        if self.h:
            load_library().mfx_db_stage_boost(self.h)

    def close(self):
        if self.h:
            load_library().mfx_db_stage_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Index:
    """Joint read+assembly k-mer count table resident in HBM."""

    def __init__(self, k, capacity_kmers, max_gb=0.0, device=0, _handle=None, seq_only=False, load_factor=0.0):
        L = load_library()
        self.k = k
        self.device = device
        if _handle is not None:
            self.h = _handle
        elif seq_only and load_factor:
            self.h = _need(L.mfx_index_create_for_seq_lf(k, int(capacity_kmers), float(max_gb), device, float(load_factor)))
        elif seq_only:
            self.h = _need(L.mfx_index_create_for_seq(k, int(capacity_kmers), float(max_gb), device))
        elif load_factor:
            self.h = _need(L.mfx_index_create_lf(k, int(capacity_kmers), float(max_gb), device, float(load_factor)))
        else:
            self.h = _need(L.mfx_index_create(k, int(capacity_kmers), float(max_gb), device))

    @staticmethod
    def for_seq(k, capacity_kmers, max_gb=0.0, device=0, load_factor=0.0):
        """a SEQUENCE-ONLY index (mfx_index_create_for_seq): claim the k-mers of the sequence first (count_asm or
        claim_seq), then add / load -- those only update the claimed k-mers.  For -hist and -dump."""
        return Index(k, capacity_kmers, max_gb=max_gb, device=device, seq_only=True, load_factor=load_factor)

    def count_claimed(self, seqs, stream=None):
        """asmV += 1 per occurrence, in `seqs`, of a k-mer claimed before (claim_seq); nothing is claimed"""
        _check(load_library().mfx_index_count_claimed(self.h, seqs.h, C.c_void_p(stream or 0)))

    def build_for_hist(self, seqs, read_db_path, minV=0, maxV=2**64 - 1):
        """count_asm(seqs) + load_db(read_db_path, 0, minV, maxV) in one call: the database crosses PCIe while the sequence's k-mers are claimed"""
        _check(load_library().mfx_index_build_for_hist(self.h, seqs.h, read_db_path.encode(), minV, maxV))

    def build_for_hist_staged(self, seqs, stage, minV=0, maxV=2**64 - 1):
        """the same from a DbStage (mfx_db_stage_begin): the database has been on its way into device memory since the stage was made"""
        _check(load_library().mfx_index_build_for_hist_staged(self.h, seqs.h, stage.h, minV, maxV))

    def load_db_staged(self, stage, side, minV=0, maxV=2**64 - 1):
        """load_db of a DbStage: only the decode + insert kernels are left to run (side 0 -readmers, 1 -seqmers)"""
        _check(load_library().mfx_index_load_db_staged(self.h, stage.h, int(side), minV, maxV))

    def claim_seq(self, seqs, stream=None):
        _check(load_library().mfx_index_claim_seq(self.h, seqs.h, C.c_void_p(stream or 0)))

    def save(self, path):
        """write the built table as a device-format image"""
        _check(load_library().mfx_index_save(self.h, path.encode()))

    @staticmethod
    def load(path, max_gb=0.0, device=0):
        h = _need(load_library().mfx_index_load(path.encode(), float(max_gb), device))
        ix = Index(0, 0, device=device, _handle=h)
        ix.k = ix.info()["k"]
        return ix

    def image_header(self):
        """geometry + filter of the built table (INDEX_HEADER_BYTES bytes), see Index.from_header"""
        buf = np.zeros(INDEX_HEADER_BYTES, dtype=np.uint8)
        _check(load_library().mfx_index_image_header(self.h, C.c_void_p(buf.ctypes.data)))
        return buf

    @staticmethod
    def from_header(header, max_gb=0.0, device=0):
        """an empty index of exactly that geometry; fill device_image() (e.g. by a broadcast), then commit()"""
        header = np.ascontiguousarray(header, dtype=np.uint8)
        h = _need(load_library().mfx_index_create_from_header(C.c_void_p(header.ctypes.data), float(max_gb), device))
        ix = Index(0, 0, device=device, _handle=h)
        ix.k = ix.info()["k"]
        return ix

    def device_image(self):
        """(lines device pointer, bytes, meta device pointer, bytes) of the table in HBM"""
        pl, pm = C.c_void_p(), C.c_void_p()
        nl, nm = C.c_uint64(), C.c_uint64()
        _check(load_library().mfx_index_device_image(self.h, C.byref(pl), C.byref(nl), C.byref(pm), C.byref(nm)))
        return pl.value, nl.value, pm.value, nm.value

    def commit(self):
        _check(load_library().mfx_index_commit(self.h))

    def replicate(self, device):
        """a copy of the built table on another device of the node (peer copy over xGMI), no second build"""
        h = _need(load_library().mfx_index_replicate(self.h, device))
        ix = Index(0, 0, device=device, _handle=h)
        ix.k = self.k
        return ix

    def replicate_many(self, devices):
        """copies on several devices at once: a doubling tree over xGMI (every device that holds the table feeds another one
        in each round, all copies of a round in flight together)"""
        devs = (C.c_int * len(devices))(*devices)
        out = (C.c_void_p * len(devices))()
        _check(load_library().mfx_index_replicate_many(self.h, devs, len(devices), out))
        res = []
        for d, h in zip(devices, out):
            ix = Index(0, 0, device=d, _handle=h)
            ix.k = self.k
            res.append(ix)
        return res

    def set_fingerprint(self, fp):
        _check(load_library().mfx_index_set_fingerprint(self.h, int(fp)))

    def origin(self):
        """(fingerprint, minV, maxV) stored with the table"""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(load_library().mfx_index_get_origin(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def add_read(self, kmers, values, minV=0, maxV=2**64 - 1):
        if isinstance(kmers, np.ndarray):
            kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
            values = np.ascontiguousarray(values, dtype=np.uint32)
        pk, dev, _k1 = _ptr(kmers)
        pv, _, _k2 = _ptr(values)
        _check(load_library().mfx_index_add_read(self.h, pk, pv, len(kmers), minV, maxV, dev))

    def add_asm(self, kmers, values):
        if isinstance(kmers, np.ndarray):
            kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
            values = np.ascontiguousarray(values, dtype=np.uint32)
        pk, dev, _k1 = _ptr(kmers)
        pv, _, _k2 = _ptr(values)
        _check(load_library().mfx_index_add_asm(self.h, pk, pv, len(kmers), dev))

    def set_shard(self, rank, nranks):
        """Sharded index: keep only the k-mers owned by `rank` of `nranks` (call before loading)."""
        _check(load_library().mfx_index_set_shard(self.h, rank, nranks))

    def load_db(self, path, side, minV=0, maxV=2**64 - 1):
        """side 0: read DB (-min/-max), side 1: assembly DB"""
        _check(load_library().mfx_index_load_db(self.h, path.encode(), side, minV, maxV))

    def count_asm(self, seqs, stream=None):
        _check(load_library().mfx_index_count_asm(self.h, seqs.h, C.c_void_p(stream or 0)))

    def count_reads(self, reads, batch_bases=0, minV=0, maxV=2**64 - 1, chunk=4096):
        """read counts straight from reads (mfx_reads_begin / add / end): the canonical k-mers of `reads` (bytes or str
        records, any case, N breaks a k-mer) are added to the read counts of the k-mers this index holds, the others are
        dropped.  A sequence-only / path-only index (k > 31: a table of the assembly's k-mers) whose read side has no counts
        yet.  Returns the counter's statistics as a dict."""
        return self._count_reads(load_library().mfx_reads_begin, reads, batch_bases, minV, maxV, chunk)

    def count_reads_all(self, reads, batch_bases=0, chunk=4096, minV=0, maxV=2**64 - 1):
        """`meryl count` of the reads on the device (mfx_reads_begin_all): every canonical k-mer of `reads` is claimed if this index
        does not hold it, and its read count grows by its occurrences; the table grows as it fills (info() shows the new capacity,
        growths() how often).  A full index, k <= 31, not sharded, whose read side has no counts yet; no Evaluator or replica of it
        may exist meanwhile.  Returns the counter's statistics as a dict (dropped == 0)."""
        return self._count_reads(load_library().mfx_reads_begin_all, reads, batch_bases, minV, maxV, chunk)

    def count_reads_range(self, reads, key_lo, key_hi, batch_bases=0, chunk=4096):
        """one pass of a count in several (mfx_reads_begin_range): as count_reads_all, for the canonical k-mers with key_lo <= k-mer < key_hi
        only.  In the statistics `kmers` is every valid k-mer of the reads and `counted` the occurrences in the range."""
        L = load_library()
        return self._count_reads(lambda h, bb: L.mfx_reads_begin_range(h, bb, int(key_lo), int(key_hi)), reads, batch_bases, 0, 2**64 - 1, chunk)

    def key_bins(self, side=0):
        """the entries with a non-zero count on `side` per top min(2k, 12) bits of their k-mer (mfx_index_key_bins): a uint64 array of
        2^min(2k, 12) bins"""
        bins = np.zeros(4096, dtype=np.uint64)
        n = C.c_uint32(0)
        _check(load_library().mfx_index_key_bins(self.h, int(side), bins.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n)))
        return bins[:n.value].copy()

    def growths(self):
        """what claiming counters did to the table (mfx_index_growths)"""
        n, b = C.c_uint64(0), C.c_uint64(0)
        s, rs = C.c_double(0), C.c_double(0)
        _check(load_library().mfx_index_growths(self.h, C.byref(n), C.byref(s), C.byref(rs), C.byref(b)))
        return {"growths": n.value, "seconds": s.value, "rehash_seconds": rs.value, "rehash_bytes": b.value}

    def write_db(self, path, side=0, streamed=False):
        """the k-mers with a non-zero count on `side` (0: reads, 1: assembly) as the sorted flat database db_write_flat makes of them
        (mfx_index_write_db); returns their number.  streamed: the blocks are coded on the device and go to disk as they are made
        (mfx_index_write_db_streamed) -- the same bytes"""
        n = C.c_uint64(0)
        L = load_library()
        _check((L.mfx_index_write_db_streamed if streamed else L.mfx_index_write_db)(self.h, int(side), str(path).encode(), C.byref(n)))
        return n.value

    def _count_reads(self, begin, reads, batch_bases, minV, maxV, chunk):
        L = load_library()
        recs = [x.encode() if isinstance(x, str) else bytes(x) for x in reads]      # (before begin: a bad record leaves the index as it was)
        r = _need(begin(self.h, int(batch_bases)))
        rc = L.mfx_reads_set_filter(r, int(minV), int(maxV))
        for o in range(0, len(recs), chunk):
            if rc:
                break
            part = recs[o:o + chunk]
            ptrs = (C.c_char_p * len(part))(*part)
            lens = (C.c_uint64 * len(part))(*[len(x) for x in part])
            try:
                rc = L.mfx_reads_add(r, ptrs, lens, len(part))
            except BaseException:
                L.mfx_reads_end(r, None)                             # (the counter is always ended: streams and pinned stages freed)
                raise
        msg = L.mfx_last_error().decode() if rc else ""
        st = _ReadsStats()
        rc_end = L.mfx_reads_end(r, C.byref(st))
        if rc:
            raise MfxError(rc, msg)
        _check(rc_end)
        return {f: getattr(st, f) for f, _ in _ReadsStats._fields_}

    def value(self, kmers):
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        r = np.zeros(len(kmers), dtype=np.uint32)
        a = np.zeros(len(kmers), dtype=np.uint32)
        _check(load_library().mfx_index_value(self.h, kmers.ctypes.data_as(C.POINTER(C.c_uint64)), len(kmers),
                                              r.ctypes.data_as(C.POINTER(C.c_uint32)), a.ctypes.data_as(C.POINTER(C.c_uint32))))
        return r, a

    def info(self):
        i = _Info()
        _check(load_library().mfx_index_get_info(self.h, C.byref(i)))
        return {"k": i.k, "canonical": bool(i.canonical), "capacity": i.capacity, "distinct": i.distinct, "bytes": i.bytes,
                "seq_only": bool(i.seq_only), "compact": bool(i.compact), "dropped": i.dropped}

    def spectrum(self, copies=4, max_mult=10000, with_entries=False):
        """the copy-number spectrum of the index's entries (mfx_spectrum_run): a (copies + 2, max_mult + 1) uint64 array -- row r:
        assembly count r (the last row: > copies), column m: read count m after -min / -max (the last column: >= max_mult);
        with_entries: also the number of counted entries"""
        img = np.zeros((int(copies) + 2, int(max_mult) + 1), dtype=np.uint64)
        n = C.c_uint64(0)
        _check(load_library().mfx_spectrum_run(self.h, int(copies), int(max_mult), img.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n)))
        return (img, n.value) if with_entries else img

    def spectrum_kernel_ms(self, copies=4, max_mult=10000, aggregate=False, reps=5):
        """diagnostic (mfx_diag_spectrum_time): the spectrum kernels' time in ms, HIP events, of each of `reps` passes"""
        ms = (C.c_float * reps)()
        _check(load_library().mfx_diag_spectrum_time(self.h, int(copies), int(max_mult), 1 if aggregate else 0, reps, ms))
        return list(ms)

    def export(self, sort=True):
        """every stored (k-mer, readV, asmV), sorted by k-mer (sort=False: table order).  k > 31: k-mers are rows
        [low 64 bits, high bits]"""
        n = self.info()["distinct"]
        if self.k > 31:
            k = np.zeros((max(n, 1), 2), dtype=np.uint64)
            r = np.zeros(max(n, 1), dtype=np.uint32)
            a = np.zeros(max(n, 1), dtype=np.uint32)
            cnt = C.c_uint64(0)
            _check(load_library().mfx_index_export(self.h, k.ctypes.data_as(C.POINTER(C.c_uint64)), r.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                   a.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(cnt)))
            k, r, a = k[:cnt.value], r[:cnt.value], a[:cnt.value]
            if not sort:
                return k, r, a
            o = np.lexsort((k[:, 0], k[:, 1]))
            return k[o], r[o], a[o]
        k = np.zeros(max(n, 1), dtype=np.uint64)
        r = np.zeros(max(n, 1), dtype=np.uint32)
        a = np.zeros(max(n, 1), dtype=np.uint32)
        cnt = C.c_uint64(0)
        _check(load_library().mfx_index_export(self.h, k.ctypes.data_as(C.POINTER(C.c_uint64)),
                                               r.ctypes.data_as(C.POINTER(C.c_uint32)), a.ctypes.data_as(C.POINTER(C.c_uint32)),
                                               C.byref(cnt)))
        if not sort:
            return k[:cnt.value], r[:cnt.value], a[:cnt.value]
        o = np.argsort(k[:cnt.value])
        return k[:cnt.value][o], r[:cnt.value][o], a[:cnt.value][o]

    def close(self):
        if getattr(self, "h", None):
            load_library().mfx_index_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


class DbWriter:
    """a k-mer database written from several tables in ascending key order (mfx_db_writer_*): append(index) per table, then close() writes
    the file db_write_flat makes of everything appended; nothing exists at `path` before.  abort() (or dropping the object) writes nothing.
    streamed: the blocks go to the spool `path`.blocks as they are made (mfx_db_writer_open_streamed) and the host keeps the directory, the
    escapes and less than one block of k-mers; close() puts header, directory, spool and escapes together -- the same bytes."""

    def __init__(self, path, k, streamed=False):
        L = load_library()
        self.h = _need((L.mfx_db_writer_open_streamed if streamed else L.mfx_db_writer_open)(str(path).encode(), int(k)))

    def append(self, index, side=0):
        """the k-mers of `index` with a non-zero count on `side` behind those held; they must start above the last one held (else MfxError,
        nothing added).  Returns their number."""
        n = C.c_uint64(0)
        _check(load_library().mfx_db_writer_append_index(self.h, index.h, int(side), C.byref(n)))
        return n.value

    def append_sorted(self, kmers, values):
        """host arrays, strictly ascending and above the last k-mer held (else MfxError, nothing added); returns their number"""
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        values = np.ascontiguousarray(values, dtype=np.uint32)
        if len(kmers) != len(values):
            raise ValueError("append_sorted: %d k-mers, %d values" % (len(kmers), len(values)))
        _check(load_library().mfx_db_writer_append_sorted(self.h, kmers.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                          values.ctypes.data_as(C.POINTER(C.c_uint32)), len(kmers)))
        return len(kmers)

    def info(self):
        """{kmers, blocks, escapes, spool_bytes, held_bytes} (mfx_db_writer_info); held_bytes: the host memory that grows with the database"""
        v = [C.c_uint64(0) for _ in range(5)]
        _check(load_library().mfx_db_writer_info(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("kmers", "blocks", "escapes", "spool_bytes", "held_bytes"), (x.value for x in v)))

    def close(self):
        n = C.c_uint64(0)
        h, self.h = self.h, None
        _check(load_library().mfx_db_writer_close(h, C.byref(n)))
        return n.value

    def abort(self):
        if getattr(self, "h", None):
            load_library().mfx_db_writer_abort(self.h)
            self.h = None

    def __del__(self):
        self.abort()


class ReadsStore:
    """the packed batches of a read set on the host (mfx_reads_store_*), 3 bits per base: parse once, count in several passes.  No device."""

    def __init__(self, k, batch_bases=0, max_bytes=0):
        self.k = int(k)
        self.h = _need(load_library().mfx_reads_store_create(self.k, int(batch_bases), int(max_bytes)))

    def add(self, reads, chunk=4096):
        """records (bytes or str) into the store; False: the store is full and incomplete from now on"""
        L = load_library()
        recs = [x.encode() if isinstance(x, str) else bytes(x) for x in reads]
        for o in range(0, len(recs), chunk):
            part = recs[o:o + chunk]
            ptrs = (C.c_char_p * len(part))(*part)
            lens = (C.c_uint64 * len(part))(*[len(x) for x in part])
            rc = L.mfx_reads_store_add(self.h, ptrs, lens, len(part))
            if rc == 1:
                return False
            _check(rc)
        return True

    def info(self):
        b, y, r, n = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        c = C.c_int(0)
        _check(load_library().mfx_reads_store_info(self.h, C.byref(b), C.byref(y), C.byref(r), C.byref(n), C.byref(c)))
        return {"batches": b.value, "bytes": y.value, "reads": r.value, "bases": n.value, "complete": bool(c.value)}

    def replay(self, index, key_range=None, update_only=False, batch_bases=0, first_batch=0, n_batches=None):
        """the store's batches through a counter of `index` (mfx_reads_replay): the claiming counter, the ranged one over key_range =
        (key_lo, key_hi), or with update_only the counter of count_reads.  Returns the counter's statistics."""
        L = load_library()
        if update_only:
            r = L.mfx_reads_begin(index.h, int(batch_bases))
        elif key_range is None:
            r = L.mfx_reads_begin_all(index.h, int(batch_bases))
        else:
            r = L.mfx_reads_begin_range(index.h, int(batch_bases), int(key_range[0]), int(key_range[1]))
        r = _need(r)
        if n_batches is None:
            n_batches = self.info()["batches"] - first_batch
        rc = L.mfx_reads_replay(r, self.h, int(first_batch), int(n_batches))
        msg = L.mfx_last_error().decode() if rc else ""
        st = _ReadsStats()
        rc_end = L.mfx_reads_end(r, C.byref(st))
        if rc:
            raise MfxError(rc, msg)
        _check(rc_end)
        return {f: getattr(st, f) for f, _ in _ReadsStats._fields_}

    def close(self):
        if getattr(self, "h", None):
            load_library().mfx_reads_store_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


class Sequences:
    """All contigs of the assembly packed into one HBM buffer."""

    def __init__(self, contigs=None, device=0, names=None, _handle=None):
        L = load_library()
        self.device = device
        if _handle is not None:
            self.h = _handle
        else:
            n = len(contigs)
            arr = (C.c_char_p * n)(*contigs)
            lens = np.array([len(c) for c in contigs], dtype=np.uint64)
            self.h = _need(L.mfx_seq_upload(device, arr, lens.ctypes.data_as(C.POINTER(C.c_uint64)), n))
        self.names = names

    @staticmethod
    def from_device(ptrs, lens, device=0, stream=None, names=None):
        L = load_library()
        n = len(ptrs)
        arr = (C.c_void_p * n)(*[int(p) for p in ptrs])
        ln = np.array(lens, dtype=np.uint64)
        h = _need(L.mfx_seq_from_device(device, arr, ln.ctypes.data_as(C.POINTER(C.c_uint64)), n, C.c_void_p(stream or 0)))
        return Sequences(device=device, names=names, _handle=h)

    @staticmethod
    def create(lens, device=0, names=None):
        """layout + device buffers of an assembly whose bases arrive later (Evaluator.hist_streamed)"""
        ln = np.array(lens, dtype=np.uint64)
        h = _need(load_library().mfx_seq_create(device, ln.ctypes.data_as(C.POINTER(C.c_uint64)), len(ln)))
        return Sequences(device=device, names=names, _handle=h)

    def replicate(self, device):
        """a copy of the packed assembly on another device of the node"""
        return Sequences(device=device, names=self.names, _handle=_need(load_library().mfx_seq_replicate(self.h, device)))

    def replicate_many(self, devices):
        """copies on several devices at once (doubling tree over xGMI); the assembly travels as its packed planes"""
        devs = (C.c_int * len(devices))(*devices)
        out = (C.c_void_p * len(devices))()
        _check(load_library().mfx_seq_replicate_many(self.h, devs, len(devices), out))
        return [Sequences(device=d, names=self.names, _handle=h) for d, h in zip(devices, out)]

    def pack(self):
        """build the packed planes (2-bit codes + validity bits) from the resident bases, on the device"""
        _check(load_library().mfx_seq_pack(self.h))

    @property
    def packed(self):
        """the evaluations read the packed planes (made once for every resident sequence; MFX_SEQ_PACK=0: not made), not one byte per base"""
        f = load_library().mfx_seq_is_packed           # (looked up here: an A/B library of older sources, MFX_LIB, has no such symbol)
        f.argtypes = [C.c_void_p]
        return bool(f(self.h))

    @property
    def ncontigs(self):
        return load_library().mfx_seq_num_contigs(self.h)

    @property
    def nbases(self):
        return load_library().mfx_seq_num_bases(self.h)

    @property
    def ntiles(self):
        return load_library().mfx_seq_num_tiles(self.h)

    def close(self):
        if getattr(self, "h", None):
            load_library().mfx_seq_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


class HistResult:
    """merfinGlobal's histogram accumulators (merfin-globals.H:184-192)."""

    def __init__(self):
        self.c = _HistResult()

    kasm = property(lambda s: s.c.kasm)
    kmissing = property(lambda s: s.c.kmissing)
    koverCpy = property(lambda s: s.c.koverCpy)

    def undr(self):
        return np.ctypeslib.as_array(self.c.undr, shape=(self.c.undrMax,)).copy()

    def over(self):
        return np.ctypeslib.as_array(self.c.over, shape=(self.c.overMax,)).copy()

    def contig_kasm(self):
        return np.ctypeslib.as_array(self.c.contig_kasm, shape=(max(self.c.ncontigs, 1),))[:self.c.ncontigs].copy()

    def contig_kmissing(self):
        return np.ctypeslib.as_array(self.c.contig_kmissing, shape=(max(self.c.ncontigs, 1),))[:self.c.ncontigs].copy()

    def add_overflow(self, records):
        """fold K* bins >= nbins (Evaluator.take_overflow / Comm.allgather_overflow: {key, occurrences} pairs, shape (n, 2)) into this result"""
        rec = np.ascontiguousarray(records, dtype=np.uint64).reshape(-1)
        if len(rec):
            _check(load_library().mfx_hist_result_add_overflow(C.byref(self.c), rec.ctypes.data_as(C.POINTER(C.c_uint64)), len(rec) // 2))
        return self

    def report(self, k, hist_path=None, summary_path=None):
        _check(load_library().mfx_hist_report(C.byref(self.c), k, hist_path.encode() if hist_path else None,
                                              summary_path.encode() if summary_path else None))

    def __del__(self):
        try:
            load_library().mfx_hist_result_free(C.byref(self.c))
        except Exception:
            pass


def result_from_counts(nbins, h_counts, kover, ncontigs):
    """(all-reduced) counts image -> HistResult; host-only, needs no device"""
    h_counts = np.ascontiguousarray(h_counts, dtype=np.uint64)
    assert len(h_counts) >= hist_words(nbins, ncontigs)
    r = HistResult()
    _check(load_library().mfx_hist_result_from_counts(nbins, h_counts.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                      float(kover), ncontigs, C.byref(r.c)))
    return r


class Router:
    """Source side of the sharded -hist: groups the k-mers of sequence tiles by owner rank."""

    def __init__(self, index, nranks, max_tiles):
        self.index = index
        self.nranks = nranks
        self.max_tiles = max_tiles
        self.h = _need(load_library().mfx_router_create(index.h, nranks, max_tiles))

    def route(self, seqs, tile_begin, tile_end, nbins, d_counts, d_keys_out, d_contigs_out, stream=None):
        p = lambda x: C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        dest = np.zeros(self.nranks, dtype=np.uint64)
        _check(load_library().mfx_route_tiles(self.h, seqs.h, tile_begin, tile_end, nbins, p(d_counts), p(d_keys_out),
                                              p(d_contigs_out), dest.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_void_p(stream or 0)))
        return dest

    def close(self):
        if getattr(self, "h", None):
            load_library().mfx_router_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


class PinnedBuffer:
    """page-locked host memory from the library (mfx_host_alloc): what a loader should read the assembly into, so that
    the streamed upload DMAs it in place.  .array is a uint8 numpy view."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.p = _need(load_library().mfx_host_alloc(self.nbytes))
        self.array = np.ctypeslib.as_array(C.cast(self.p, C.POINTER(C.c_uint8)), shape=(max(self.nbytes, 1),))[:self.nbytes]

    def close(self):
        if getattr(self, "p", None):
            self.array = None
            load_library().mfx_host_free(self.p)
            self.p = None

    def __del__(self):
        self.close()


def hist_multi(evaluators, sequences):
    """-hist over several devices driven by this one process (mfx_hist_run_multi): evaluators[d] / sequences[d] are
    replicas on device d; slot d evaluates the block-cyclic share d of N of the tiles, all at once."""
    n = len(evaluators)
    assert n == len(sequences) and n >= 1
    ev = (C.c_void_p * n)(*[e.h for e in evaluators])
    sq = (C.c_void_p * n)(*[s.h for s in sequences])
    r = HistResult()
    _check(load_library().mfx_hist_run_multi(ev, sq, n, C.byref(r.c)))
    return r


def _host_ptrs(host_contigs):
    """(ctypes void* array, objects to keep alive) of bytes / numpy uint8 arrays / PinnedBuffer views, one per contig"""
    n = len(host_contigs)
    keep = []
    ptrs = (C.c_void_p * max(n, 1))()
    for i, c in enumerate(host_contigs):
        if isinstance(c, (bytes, bytearray)):
            b = C.c_char_p(bytes(c))
            keep.append(b)
            ptrs[i] = C.cast(b, C.c_void_p).value
        else:
            a = np.ascontiguousarray(c, dtype=np.uint8)
            keep.append(a)
            ptrs[i] = a.ctypes.data
    return ptrs, keep


def hist_streamed_multi(evaluators, sequences, host_contigs):
    """SURVEY 8(d)'s evaluate phase over several devices driven by this one process (mfx_hist_run_streamed_multi): slot d gets,
    through its own copy stream, only the packed planes of its contiguous share of the tiles and evaluates them as they land.
    sequences[d] = Sequences.create(lens, device=d): one object per slot (it holds the slot's part afterwards)."""
    n = len(evaluators)
    assert n == len(sequences) and n >= 1
    ev = (C.c_void_p * n)(*[e.h for e in evaluators])
    sq = (C.c_void_p * n)(*[s.h for s in sequences])
    ptrs, keep = _host_ptrs(host_contigs)
    r = HistResult()
    _check(load_library().mfx_hist_run_streamed_multi(ev, sq, n, ptrs, C.byref(r.c)))
    return r


def stream_share(ntiles, rank, nranks):
    """the tiles [begin, end) rank `rank` of `nranks` streams (mfx_hist_stream_share)"""
    a, b = C.c_uint64(0), C.c_uint64(0)
    _check(load_library().mfx_hist_stream_share(ntiles, rank, nranks, C.byref(a), C.byref(b)))
    return a.value, b.value


def hist_sharded(evaluators, routers, sequences):
    """-hist over an index sharded across the slots of ONE process (mfx_hist_run_sharded): slot d = evaluator + router on
    shard d of N, plus the packed assembly on that shard's device"""
    n = len(evaluators)
    assert n == len(routers) == len(sequences) and n >= 1
    ev = (C.c_void_p * n)(*[e.h for e in evaluators])
    ro = (C.c_void_p * n)(*[r.h for r in routers])
    sq = (C.c_void_p * n)(*[s.h for s in sequences])
    r = HistResult()
    _check(load_library().mfx_hist_run_sharded(ev, ro, sq, n, C.byref(r.c)))
    return r


def track_write(windows, seqs, names, window, tsv_path=None, bedgraph_path=None):
    """the records of Evaluator.track as text (mfx_track_write; host only): a table of every window with k-mers and / or a
    bedGraph track of the mean K*; .gz / .bz2 / .xz names are compressed"""
    w = np.ascontiguousarray(windows, dtype=TRACK_DTYPE)
    nm = (C.c_char_p * max(len(names), 1))(*[x.encode() if isinstance(x, str) else x for x in names])
    _check(load_library().mfx_track_write(C.c_void_p(w.ctypes.data), len(w), seqs.h, nm, int(window),
                                          tsv_path.encode() if tsv_path else None, bedgraph_path.encode() if bedgraph_path else None))


def _regions_opts(kstar, gap, min_kmers):
    if not (0 <= int(gap) < 2**64 and 0 <= int(min_kmers) < 2**64):
        raise MfxError(-1, "regions: gap and min_kmers are integers in [0, 2^64)")
    return _RegionsOpts(float(kstar), int(gap), int(min_kmers))


def regions_write(regions, seqs, names, k, bed_path):
    """the records of Evaluator.regions as BED text (mfx_regions_write; host only): a header line, then chrom, the base span
    [start, end - 1 + k), the class, n_kmers, mean readK, mean asmK and the extreme K*; .gz / .bz2 / .xz names are compressed"""
    r = np.ascontiguousarray(regions, dtype=REGION_DTYPE)
    nm = (C.c_char_p * max(len(names), 1))(*[x.encode() if isinstance(x, str) else x for x in names])
    _check(load_library().mfx_regions_write(C.c_void_p(r.ctypes.data), len(r), seqs.h, nm, int(k), bed_path.encode()))


def regions_from_planes_host(planes, contig_lens, gap=0, min_kmers=1):
    """the steps of Evaluator.regions between its two passes, on the host, over caller-made class planes (mfx_regions_from_planes_host):
    planes is a uint64 array [3][ntiles * 64], ntiles = sum(ceil(len / 4096)); the records come back with their sums at 0"""
    planes = np.ascontiguousarray(planes, dtype=np.uint64)
    lens = np.ascontiguousarray(contig_lens, dtype=np.uint64)
    ntiles = int(sum((int(x) + 4095) // 4096 for x in lens))
    if planes.size != 3 * 64 * ntiles:
        raise MfxError(-1, "regions_from_planes_host: %d words for %d tiles (3 x 64 each)" % (planes.size, ntiles))
    o = _regions_opts(1.0, gap, min_kmers)
    L = load_library()
    n = C.c_uint64(0)
    lp = lens.ctypes.data_as(C.POINTER(C.c_uint64))
    _check(L.mfx_regions_from_planes_host(C.c_void_p(planes.ctypes.data), lp, len(lens), C.byref(o), None, 0, C.byref(n)))
    out = np.zeros(max(n.value, 1), dtype=REGION_DTYPE)
    _check(L.mfx_regions_from_planes_host(C.c_void_p(planes.ctypes.data), lp, len(lens), C.byref(o), C.c_void_p(out.ctypes.data), n.value, C.byref(n)))
    return out[:n.value]


def _phase_opts(switches, range_):
    if not (0 <= int(switches) < 2**64 and 0 <= int(range_) < 2**64):
        raise MfxError(-1, "phase: switches and range are integers in [0, 2^64)")
    return _PhaseOpts(int(switches), int(range_))


def phase_write(blocks, contig_counts, seqs, names, k, stem, switches=100, range_=20000):
    """the records and per-contig counts of Evaluator.phase as text (mfx_phase_write; host only): <stem>.phased_block.bed,
    <stem>.hapmers.count and <stem>.phased_block.stats; a stem ending in .gz / .bz2 / .xz compresses them (the suffix stays last)"""
    b = np.ascontiguousarray(blocks, dtype=PHASE_DTYPE)
    cc = np.ascontiguousarray(contig_counts, dtype=np.uint64)
    nm = (C.c_char_p * max(len(names), 1))(*[x.encode() if isinstance(x, str) else x for x in names])
    o = _phase_opts(switches, range_)
    _check(load_library().mfx_phase_write(C.c_void_p(b.ctypes.data), len(b), C.c_void_p(cc.ctypes.data), seqs.h, nm, int(k), C.byref(o), stem.encode()))


def phase_from_planes_host(planes, contig_lens, k, switches=100, range_=20000):
    """pass 2 of Evaluator.phase on the host over caller-made haplotype planes (mfx_phase_from_planes_host): planes is a uint64 array
    [2][ntiles * 64], ntiles = sum(ceil(len / 4096)); plane 0 flags the markers of A, plane 1 those of B"""
    planes = np.ascontiguousarray(planes, dtype=np.uint64)
    lens = np.ascontiguousarray(contig_lens, dtype=np.uint64)
    ntiles = int(sum((int(x) + 4095) // 4096 for x in lens))
    if planes.size != 2 * 64 * ntiles:
        raise MfxError(-1, "phase_from_planes_host: %d words for %d tiles (2 x 64 each)" % (planes.size, ntiles))
    o = _phase_opts(switches, range_)
    L = load_library()
    n = C.c_uint64(0)
    lp = lens.ctypes.data_as(C.POINTER(C.c_uint64))
    _check(L.mfx_phase_from_planes_host(C.c_void_p(planes.ctypes.data), lp, len(lens), int(k), C.byref(o), None, 0, C.byref(n)))
    out = np.zeros(max(n.value, 1), dtype=PHASE_DTYPE)
    _check(L.mfx_phase_from_planes_host(C.c_void_p(planes.ctypes.data), lp, len(lens), int(k), C.byref(o), C.c_void_p(out.ctypes.data), n.value, C.byref(n)))
    return out[:n.value]


E_NODATA = -10


class Binner:
    """the per-read hap-mer counter of -bin (mfx_bin_*): records go in with add(), their counts come out of take() in input order.  The
    index behind the evaluator holds set A on its read side and set B on its assembly side, as for Evaluator.phase."""

    def __init__(self, evaluator, batch_bases=0):
        self.h = _need(load_library().mfx_bin_begin(evaluator.h if evaluator is not None else None, int(batch_bases)))
        self._ev = evaluator                                         # (the index must outlive the binner)

    def add(self, reads):
        recs = [x.encode() if isinstance(x, str) else bytes(x) for x in reads]
        ptrs = (C.c_char_p * len(recs))(*recs)
        lens = (C.c_uint64 * len(recs))(*[len(x) for x in recs])
        _check(load_library().mfx_bin_add(self.h, ptrs, lens, len(recs)))

    def flush(self):
        _check(load_library().mfx_bin_flush(self.h))

    def ready(self):
        return load_library().mfx_bin_ready(self.h)

    def take(self, cap):
        """the next min(cap, ready()) records: a uint32 array [n, 4] of k-mers, A only, B only, shared"""
        out = np.zeros((max(int(cap), 1), 4), dtype=np.uint32)
        n = C.c_uint64(0)
        _check(load_library().mfx_bin_take(self.h, C.c_void_p(out.ctypes.data), int(cap), C.byref(n)))
        return out[:n.value]

    def end(self):
        """flushes and frees the binner; the statistics as a dict"""
        h, self.h = self.h, None
        st = _BinStats()
        _check(load_library().mfx_bin_end(h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in _BinStats._fields_}

    def close(self):
        if getattr(self, "h", None):
            h, self.h = self.h, None
            load_library().mfx_bin_end(h, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bin_classify(records, norm_a, norm_b, ratio_milli=1000, min_hits=1):
    """the class rule of -bin over the records of Evaluator.bin_reads (mfx_bin_classify; host only, integers only): a uint8 array of
    0 (A), 1 (B), 2 (unknown).  The rule is this project's own, in the spirit of Canu's haplotype split; not validated against Canu."""
    r = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, 4)
    cls = np.zeros(max(len(r), 1), dtype=np.uint8)
    o = _BinOpts(int(norm_a), int(norm_b), int(ratio_milli), int(min_hits))
    _check(load_library().mfx_bin_classify(C.c_void_p(r.ctypes.data), len(r), C.byref(o), C.c_void_p(cls.ctypes.data)))
    return cls[:len(r)]


def bin_plan_host(lens, k, batch_bases=0):
    """the pieces records of these lengths are cut into by the batcher of -bin and the read counters (mfx_bin_plan_host; host only): a
    uint64 array [n_pieces, 4] of batch, record, first position in the batch, length"""
    L = load_library()
    lens = np.ascontiguousarray(lens, dtype=np.uint64)
    lp = lens.ctypes.data_as(C.POINTER(C.c_uint64))
    n = C.c_uint64(0)
    _check(L.mfx_bin_plan_host(lp, len(lens), int(k), int(batch_bases), None, 0, C.byref(n)))
    out = np.zeros((max(n.value, 1), 4), dtype=np.uint64)
    _check(L.mfx_bin_plan_host(lp, len(lens), int(k), int(batch_bases), C.c_void_p(out.ctypes.data), n.value, C.byref(n)))
    return out[:n.value]


def spectrum_peak(row):
    """the haploid peak of one spectrum row of max_mult + 1 cells (mfx_spectrum_peak; host only, exact): a dict of valley,
    main_peak, haploid_peak and count_at_peak, or None when the rule finds no peak"""
    row = np.ascontiguousarray(row, dtype=np.uint64)
    out = _SpectrumPeak()
    rc = load_library().mfx_spectrum_peak(row.ctypes.data_as(C.POINTER(C.c_uint64)), len(row) - 1, C.byref(out))
    if rc == E_NODATA:
        return None
    _check(rc)
    return {"valley": out.valley, "main_peak": out.main_peak, "haploid_peak": out.haploid_peak, "count_at_peak": out.count_at_peak}


def spectrum_write(img, path, with_read_only=True):
    """a spectrum image as text (mfx_spectrum_write; host only): Copies, kmer_multiplicity, Count per non-zero cell; .gz / .bz2 /
    .xz names are compressed.  The layout is unvalidated against Merqury."""
    img = np.ascontiguousarray(img, dtype=np.uint64)
    _check(load_library().mfx_spectrum_write(img.ctypes.data_as(C.POINTER(C.c_uint64)), img.shape[0] - 2, img.shape[1] - 1,
                                             1 if with_read_only else 0, path.encode() if isinstance(path, str) else path))


def pack_bases(seq):
    """host-side encoding of the packed sequence transport: bytes -> (codes uint64[ceil(n/32)], valid uint32[ceil(n/32)])"""
    src = np.frombuffer(bytes(seq), dtype=np.uint8)
    nw = (len(src) + 31) // 32
    codes = np.zeros(max(nw, 1), dtype=np.uint64)
    valid = np.zeros(max(nw, 1), dtype=np.uint32)
    load_library().mfx_pack_bases(C.c_void_p(src.ctypes.data), len(src), C.c_void_p(codes.ctypes.data), C.c_void_p(valid.ctypes.data))
    return codes[:nw], valid[:nw]


def dump_values_sharded(evaluators, sequences, contig, pos_begin, pos_end):
    """(readV, asmV) per k-mer start over an index sharded across the slots (mfx_dump_values_sharded)"""
    ns = len(evaluators)
    assert ns == len(sequences) and ns >= 1
    ev = (C.c_void_p * ns)(*[e.h for e in evaluators])
    sq = (C.c_void_p * ns)(*[s.h for s in sequences])
    n = pos_end - pos_begin
    r = np.zeros(max(n, 1), dtype=np.uint32)
    a = np.zeros(max(n, 1), dtype=np.uint32)
    ka, km = C.c_uint64(0), C.c_uint64(0)
    _check(load_library().mfx_dump_values_sharded(ev, sq, ns, contig, pos_begin, pos_end, r.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                  a.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(ka), C.byref(km)))
    return r[:n], a[:n], ka.value, km.value


def dump_contig_sharded(evaluators, sequences, contig, name, path, append=False):
    ns = len(evaluators)
    ev = (C.c_void_p * ns)(*[e.h for e in evaluators])
    sq = (C.c_void_p * ns)(*[s.h for s in sequences])
    ka, km = C.c_uint64(0), C.c_uint64(0)
    _check(load_library().mfx_dump_contig_sharded(ev, sq, ns, contig, name.encode(), path.encode(), 1 if append else 0,
                                                  C.byref(ka), C.byref(km)))
    return ka.value, km.value


def variants_sharded(evaluators, mode, vcf_path, names, contigs, out_path, comb=15, nosplit=False, debug_path=None, log_path=None):
    """the variant modes over an index sharded across the slots (mfx_variants_run_sharded); returns clusters evaluated"""
    ns = len(evaluators)
    ev = (C.c_void_p * ns)(*[e.h for e in evaluators])
    n = len(contigs)
    nm = (C.c_char_p * n)(*[x.encode() for x in names])
    arr = (C.c_char_p * n)(*contigs)
    lens = np.array([len(c) for c in contigs], dtype=np.uint64)
    o = _VarOpts(VARIANT_MODES[mode], comb, 1 if nosplit else 0, debug_path.encode() if debug_path else None)
    ncl = C.c_uint64(0)
    _check(load_library().mfx_variants_run_sharded(ev, ns, vcf_path.encode(), nm, arr, lens.ctypes.data_as(C.POINTER(C.c_uint64)), n,
                                                   C.byref(o), out_path.encode(), log_path.encode() if log_path else None, C.byref(ncl)))
    return ncl.value


COMM_ID_BYTES = 128          # MFX_COMM_ID_BYTES


class Comm:
    """One rank of the multi-process -hist: RCCL communicator + the path's collective (csrc/mfx_comm.cpp)."""

    @staticmethod
    def unique_id():
        buf = np.zeros(COMM_ID_BYTES, dtype=np.uint8)
        _check(load_library().mfx_comm_unique_id(C.c_void_p(buf.ctypes.data)))
        return buf

    def __init__(self, uid, rank, nranks, device=0):
        uid = np.ascontiguousarray(uid, dtype=np.uint8)
        assert len(uid) == COMM_ID_BYTES
        self.rank, self.nranks, self.device = rank, nranks, device
        self.h = _need(load_library().mfx_comm_create(C.c_void_p(uid.ctypes.data), rank, nranks, device))

    def hist_allreduce(self, ev, d_counts, d_kover, ncontigs, stream=None):
        """counts image + koverCpy of every rank -> the global ones, in place on every rank (async on `stream`)"""
        p = lambda x: C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        _check(load_library().mfx_hist_allreduce(self.h, p(d_counts), p(d_kover), ev.nbins, ncontigs, C.c_void_p(stream or 0)))

    def barrier(self, stream=None):
        """every rank has arrived and `stream` has drained"""
        _check(load_library().mfx_comm_barrier(self.h, C.c_void_p(stream or 0)))

    def allgather_overflow(self, ev, cap=1 << 20, stream=None):
        """the far K* bins of ALL ranks as {key, occurrences} pairs, shape (n, 2) (collective; call on every rank when the reduced
        image's novf word is non-zero)"""
        rec = np.zeros(2 * cap, dtype=np.uint64)
        n = C.c_uint64(0)
        _check(load_library().mfx_hist_allgather_overflow(self.h, ev.h, rec.ctypes.data_as(C.POINTER(C.c_uint64)), cap, C.byref(n),
                                                          C.c_void_p(stream or 0)))
        return rec[:2 * n.value].reshape(-1, 2)

    def exchange_counts(self, send_counts, stream=None):
        """what every rank will send to this one (all-gather of the count rows; synchronises `stream`)"""
        sc = np.ascontiguousarray(send_counts, dtype=np.uint64)
        assert len(sc) == self.nranks
        rc = np.zeros(self.nranks, dtype=np.uint64)
        _check(load_library().mfx_comm_exchange_counts(self.h, sc.ctypes.data_as(C.POINTER(C.c_uint64)), rc.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                       C.c_void_p(stream or 0)))
        return rc

    def alltoallv(self, d_send, send_counts, d_recv, recv_counts, elem_bytes, stream=None):
        """group r of d_send -> rank r, received groups in source-rank order (device buffers; async on `stream`)"""
        p = lambda x: C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        sc = np.ascontiguousarray(send_counts, dtype=np.uint64)
        rc = np.ascontiguousarray(recv_counts, dtype=np.uint64)
        _check(load_library().mfx_comm_alltoallv(self.h, p(d_send), sc.ctypes.data_as(C.POINTER(C.c_uint64)), p(d_recv),
                                                 rc.ctypes.data_as(C.POINTER(C.c_uint64)), elem_bytes, C.c_void_p(stream or 0)))

    def close(self):
        if getattr(self, "h", None):
            load_library().mfx_comm_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


def hist_parts(evaluators, sequences, contig_ids, ncontigs_total):
    """mfx_hist_run_parts: slot d evaluates its contigs (sequences[d], numbered contig_ids[d] in the whole assembly) on its own index"""
    n = len(evaluators)
    evs = (C.c_void_p * n)(*[e.h for e in evaluators])
    sqs = (C.c_void_p * n)(*[s.h for s in sequences])
    keep = [np.ascontiguousarray(ids, dtype=np.uint32) for ids in contig_ids]
    idp = (C.POINTER(C.c_uint32) * n)(*[k.ctypes.data_as(C.POINTER(C.c_uint32)) for k in keep])
    r = HistResult()
    _check(load_library().mfx_hist_run_parts(evs, sqs, idp, n, int(ncontigs_total), C.byref(r.c)))
    return r


def stream_rates(src, threads, device=0):
    """(GB/s `threads` host threads encode `src` -- a PinnedBuffer view or any contiguous uint8 array -- at, GB/s the device's link moves it at: 0 when
    src is not pinned): the two rates a streamed run's transport is chosen from (mfx_diag_stream_rates)"""
    a = np.ascontiguousarray(src)
    enc, link = C.c_double(0), C.c_double(0)
    _check(load_library().mfx_diag_stream_rates(device, C.c_void_p(a.ctypes.data), a.nbytes, threads, C.byref(enc), C.byref(link)))
    return enc.value, link.value


def gather_rate(table_bytes, device=0):
    """diagnostic: random 128-byte lines per second the device's HBM delivers over a table of that size (mfx_diag_gather_rate)"""
    out = C.c_double(0.0)
    _check(load_library().mfx_diag_gather_rate(device, int(table_bytes), C.byref(out)))
    return out.value


def _vp(a):
    return C.c_void_p(a.ctypes.data if a.size else 0)


class TraverseTables:
    """A batch of variant clusters as the tables the device traverse reads (TRV_*_DTYPE arrays + window / allele text)."""

    def __init__(self, clusters, variants, alleles, win_text, al_text, text_end, path_cap, row_cap):
        self.cl = np.ascontiguousarray(clusters, dtype=TRV_CLUSTER_DTYPE)
        self.var = np.ascontiguousarray(variants, dtype=TRV_VARIANT_DTYPE)
        self.al = np.ascontiguousarray(alleles, dtype=TRV_ALLELE_DTYPE)
        self.win = np.frombuffer(bytes(win_text), dtype=np.uint8)
        self.alt = np.frombuffer(bytes(al_text), dtype=np.uint8)
        self.text_end, self.path_cap, self.row_cap = int(text_end), int(path_cap), int(row_cap)

    def args(self):
        return [_vp(self.cl), len(self.cl), _vp(self.var), len(self.var), _vp(self.al), len(self.al), _vp(self.win), len(self.win),
                _vp(self.alt), len(self.alt), self.text_end, self.path_cap, self.row_cap]


class PathTable:
    """host-enumerated paths inside their text (mfx_debug_score_paths): off / len / nv / voff / cfirst per path, gt / vidx / vlen rows"""

    def __init__(self, text=b"", off=(), plen=(), nv=(), voff=(), cfirst=(), gt=(), vidx=(), vlen=()):
        self.text = np.frombuffer(bytes(text), dtype=np.uint8)
        self.off = np.ascontiguousarray(off, dtype=np.uint64)
        self.len = np.ascontiguousarray(plen, dtype=np.uint32)
        self.nv = np.ascontiguousarray(nv, dtype=np.uint32)
        self.voff = np.ascontiguousarray(voff, dtype=np.uint64)
        self.cfirst = np.ascontiguousarray(cfirst, dtype=np.uint64)
        self.gt = np.ascontiguousarray(gt, dtype=np.int32)
        self.vidx = np.ascontiguousarray(vidx, dtype=np.uint32)
        self.vlen = np.ascontiguousarray(vlen, dtype=np.uint32)
        assert len(self.off) == len(self.len) == len(self.nv) == len(self.voff) == len(self.cfirst)
        assert len(self.gt) == len(self.vidx) == len(self.vlen)

    def args(self):
        return [_vp(self.text), len(self.text), len(self.off), len(self.gt), _vp(self.off), _vp(self.len), _vp(self.nv), _vp(self.voff),
                _vp(self.cfirst), _vp(self.gt), _vp(self.vidx), _vp(self.vlen)]


def _trv_outputs(t):
    o = {"np": np.zeros(len(t.cl), dtype=np.uint32), "status": np.zeros(len(t.cl), dtype=np.uint32),
         "text": np.full(max(t.text_end, 1), 10, dtype=np.uint8),
         "p_off": np.zeros(max(t.path_cap, 1), dtype=np.uint64), "p_len": np.zeros(max(t.path_cap, 1), dtype=np.uint32),
         "p_nv": np.zeros(max(t.path_cap, 1), dtype=np.uint32), "p_voff": np.zeros(max(t.path_cap, 1), dtype=np.uint64),
         "p_cfirst": np.zeros(max(t.path_cap, 1), dtype=np.uint64), "gt": np.zeros(max(t.row_cap, 1), dtype=np.int32),
         "vidx": np.zeros(max(t.row_cap, 1), dtype=np.uint32), "vlen": np.zeros(max(t.row_cap, 1), dtype=np.uint32)}
    order = ["np", "status", "text", "p_off", "p_len", "p_nv", "p_voff", "p_cfirst", "gt", "vidx", "vlen"]
    return o, [C.c_void_p(o[n].ctypes.data) for n in order]


def _trv_trim(o, t):
    o["text"] = o["text"][:t.text_end]
    for n in ("p_off", "p_len", "p_nv", "p_voff", "p_cfirst"):
        o[n] = o[n][:t.path_cap]
    for n in ("gt", "vidx", "vlen"):
        o[n] = o[n][:t.row_cap]
    return o


def debug_traverse_host(tables):
    """test hook: the shared traverse, one thread, on the host (mfx_debug_traverse_host; needs no GPU).  Returns a dict of arrays:
    np, status [ncl]; text [text_end] ('\\n' where nothing was written); p_off, p_len, p_nv, p_voff, p_cfirst [path_cap]; gt, vidx,
    vlen [row_cap]"""
    o, ptrs = _trv_outputs(tables)
    _check(load_library().mfx_debug_traverse_host(*(tables.args() + ptrs)))
    return _trv_trim(o, tables)


class LoadedVcf:
    """a VCF read and parsed ahead of its run (mfx_vcf_load): no device involved"""

    def __init__(self, path):
        self.h = _need(load_library().mfx_vcf_load(path.encode()))

    def prepare(self, k, mode, names, contigs, comb=15, nosplit=False, debug_path=None):
        """the clusters merged and their allele combinations enumerated and packed ahead of the run (mfx_vcf_prepare: host work, no
        index, no device); Evaluator.variants_loaded on this handle with the same k / comb / nosplit / contigs then starts at the lookups"""
        n = len(contigs)
        nm = (C.c_char_p * n)(*[x.encode() for x in names])
        arr = (C.c_char_p * n)(*contigs)
        lens = np.array([len(c) for c in contigs], dtype=np.uint64)
        o = _VarOpts(VARIANT_MODES[mode], comb, 1 if nosplit else 0, debug_path.encode() if debug_path else None)
        _check(load_library().mfx_vcf_prepare(self.h, int(k), nm, arr, lens.ctypes.data_as(C.POINTER(C.c_uint64)), n, C.byref(o)))

    def prepare_path_index(self, k, mode, names, contigs, comb=15, nosplit=False, debug_path=None, max_gb=0.0, device=0, load_factor=0.0):
        """prepare + the path-only index in one pass (mfx_vcf_prepare_path_index): the claimed Index (load the databases next), or None when
        this call set cannot have one (the handle is prepared either way)"""
        n = len(contigs)
        nm = (C.c_char_p * n)(*[x.encode() for x in names])
        arr = (C.c_char_p * n)(*contigs)
        lens = np.array([len(c) for c in contigs], dtype=np.uint64)
        o = _VarOpts(VARIANT_MODES[mode], comb, 1 if nosplit else 0, debug_path.encode() if debug_path else None)
        h = C.c_void_p(None)
        _check(load_library().mfx_vcf_prepare_path_index(self.h, int(k), nm, arr, lens.ctypes.data_as(C.POINTER(C.c_uint64)), n, C.byref(o), float(max_gb), int(device),
                                                         float(load_factor), C.byref(h)))
        if not h.value:
            return None
        ix = Index(0, 0, device=device, _handle=h.value)
        ix.k = int(k)
        return ix

    def path_bound(self):
        """k-mer positions of all path text of the prepared call set: the capacity of its path-only index (mfx_vcf_path_bound)"""
        n = C.c_uint64(0)
        _check(load_library().mfx_vcf_path_bound(self.h, C.byref(n)))
        return n.value

    def claim_paths(self, index):
        """the k-mers of every path claimed on a sequence-only index (Index.for_sequence): the PATH-ONLY index of the variant modes
        (mfx_index_claim_paths); the databases then update those k-mers only and Evaluator.variants_loaded on this handle runs on it"""
        n = C.c_uint64(0)
        _check(load_library().mfx_index_claim_paths(index.h, self.h, C.byref(n)))
        return n.value

    def close(self):
        if self.h:
            load_library().mfx_vcf_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Evaluator:
    """K* parameters bound to an Index; runs -hist / -dump / -completeness."""

    def __init__(self, index, kparams, nbins=0):
        self.index = index
        self.kp = kparams
        self.h = _need(load_library().mfx_eval_create(index.h, C.byref(kparams.c), nbins))

    @property
    def nbins(self):
        return load_library().mfx_eval_nbins(self.h)

    def debug(self, on=True):
        """test hook: -hist launches run the DEBUG instance of the kernel (probe path counters) where one exists"""
        _check(load_library().mfx_eval_debug_enable(self.h, 1 if on else 0))

    def debug_counters(self):
        """how the probe's queries that left the one-load path ended (cleared): first_pass / second_pass (cooperative passes over the home
        line / the next candidate line), side_table (a saturated count field), line_scans (further candidate lines: listed for
        mfx_hist_rest_kernel), side_not_in_two_slots (saturated, not in slot 0 / 1 of its side-table line: listed), ended_per_lane (no
        list, or the list was full: scanned for by the lane itself).  first_pass counts every query that was not in its first mini-bucket;
        second_bucket of them ended in the second mini-bucket of their order, per lane, and never reached a cooperative pass"""
        out = np.zeros(8, dtype=np.uint64)
        _check(load_library().mfx_eval_debug_counters(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return {"first_pass": int(out[0]), "second_pass": int(out[1]), "side_table": int(out[2]), "line_scans": int(out[3]),
                "side_not_in_two_slots": int(out[4]), "ended_per_lane": int(out[5]),
                "second_bucket": int(out[6])}

    def debug_worklist(self, mode=1, segcap=0):
        """test hook: the worklist of this evaluator's later -hist launches -- mode 0 none, 1 the default sizing, 2 segments of at most
        `segcap` entries in the default's allocation (mfx_eval_debug_worklist)"""
        _check(load_library().mfx_eval_debug_worklist(self.h, mode, segcap))

    def debug_worklist_read(self, slot=0):
        """the list of the last launch of launch slot `slot`, read back after a device synchronise: (segs, segcap, counts[segs],
        entries) with entries a WORKLIST_DTYPE array, segment after segment (segment g: entries[counts[:g].sum():][:counts[g]]);
        (0, 0, empty, empty) when that launch had no list"""
        L = load_library()
        segs, segcap, n = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
        _check(L.mfx_eval_debug_worklist_read(self.h, slot, C.byref(segs), C.byref(segcap), None, 0, None, 0, C.byref(n)))
        counts = np.zeros(segs.value, dtype=np.uint64)
        ent = np.zeros(n.value, dtype=WORKLIST_DTYPE)
        _check(L.mfx_eval_debug_worklist_read(self.h, slot, C.byref(segs), C.byref(segcap), counts.ctypes.data_as(C.POINTER(C.c_uint64)), len(counts),
                                              C.c_void_p(ent.ctypes.data), len(ent), C.byref(n)))
        assert n.value == len(ent) and segs.value == len(counts)
        return segs.value, segcap.value, counts, ent

    def hist(self, seqs):
        r = HistResult()
        _check(load_library().mfx_hist_run(self.h, seqs.h, C.byref(r.c)))
        return r

    def hist_streamed(self, seqs, host_contigs):
        """-hist with the upload inside (SURVEY 8d's evaluate phase): `seqs` = Sequences.create(lens); host_contigs =
        bytes / numpy uint8 arrays / PinnedBuffer views, one per contig.  Chunked H2D overlapped with the kernel."""
        ptrs, keep = _host_ptrs(host_contigs)
        r = HistResult()
        _check(load_library().mfx_hist_run_streamed(self.h, seqs.h, ptrs, C.byref(r.c)))
        return r

    def hist_streamed_range(self, seqs, host_contigs, tile_begin, tile_end, d_counts, d_kover):
        """one rank's share of a streamed -hist (mfx_hist_run_streamed_range): tiles [tile_begin, tile_end) encoded, uploaded and
        evaluated, ADDED to the caller's device image / koverCpy; returns when the device is done"""
        ptrs, keep = _host_ptrs(host_contigs)
        pc = d_counts.data_ptr() if hasattr(d_counts, "data_ptr") else int(d_counts)
        pk = d_kover.data_ptr() if hasattr(d_kover, "data_ptr") else int(d_kover)
        _check(load_library().mfx_hist_run_streamed_range(self.h, seqs.h, ptrs, tile_begin, tile_end, C.c_void_p(pc), C.c_void_p(pk)))

    def hist_launch(self, seqs, tile_begin, tile_end, d_counts, d_kover, stream=None):
        """Asynchronous accumulate into caller-owned device buffers (torch tensors or raw pointers)."""
        pc = d_counts.data_ptr() if hasattr(d_counts, "data_ptr") else int(d_counts)
        pk = d_kover.data_ptr() if hasattr(d_kover, "data_ptr") else int(d_kover)
        _check(load_library().mfx_hist_launch(self.h, seqs.h, tile_begin, tile_end, C.c_void_p(pc), C.c_void_p(pk),
                                              C.c_void_p(stream or 0)))

    def hist_launch_cyclic(self, seqs, rank, nranks, d_counts, d_kover, block_tiles=256, stream=None):
        """the block-cyclic share of `rank`: blocks of `block_tiles` tiles dealt round-robin to the ranks"""
        p = lambda x: C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        _check(load_library().mfx_hist_launch_cyclic(self.h, seqs.h, rank, nranks, block_tiles, p(d_counts), p(d_kover),
                                                     C.c_void_p(stream or 0)))

    def result_from_counts(self, h_counts, kover, ncontigs):
        return result_from_counts(self.nbins, h_counts, kover, ncontigs)

    def take_overflow(self, cap=1 << 20):
        """the K* bins beyond the dense image seen by this evaluator's launches since the last call, as {key (bit 63: `over`; low
        bits: bin index), occurrences} pairs, shape (n, 2), sorted by key; the evaluator's table is emptied"""
        rec = np.zeros(2 * cap, dtype=np.uint64)
        n = C.c_uint64(0)
        _check(load_library().mfx_hist_take_overflow(self.h, rec.ctypes.data_as(C.POINTER(C.c_uint64)), cap, C.byref(n)))
        return rec[:2 * n.value].reshape(-1, 2)

    def hist_keys_launch(self, d_keys, d_contigs, n, ncontigs, d_counts, d_kover, stream=None):
        """Owner side of the sharded -hist: probe/K*/bin n received canonical k-mers (device buffers)."""
        p = lambda x: C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        _check(load_library().mfx_hist_keys_launch(self.h, p(d_keys), p(d_contigs), n, ncontigs, p(d_counts), p(d_kover),
                                                   C.c_void_p(stream or 0)))

    def debug_score_paths(self, paths, need_dk=True):
        """test hook: varMer::score of host-enumerated paths on the device (mfx_debug_score_paths) -> (numM, totdk)"""
        n = len(paths.off)
        numM = np.zeros(max(n, 1), dtype=np.uint32)
        totdk = np.zeros(max(n, 1), dtype=np.float64)
        _check(load_library().mfx_debug_score_paths(self.h, *(paths.args() + [1 if need_dk else 0, C.c_void_p(numM.ctypes.data), C.c_void_p(totdk.ctypes.data)])))
        return numM[:n], totdk[:n]

    def debug_score_paths_trv(self, paths, tables, need_dk=True):
        """test hook: the clusters of `tables` enumerated and scored on the device behind the host part `paths` (PathTable, may be
        empty): mfx_debug_score_paths_trv.  Returns debug_traverse_host's dict (the device part; text = the whole batch text) plus
        numM, totdk [host paths + path_cap]"""
        n = len(paths.off) + tables.path_cap
        numM = np.zeros(max(n, 1), dtype=np.uint32)
        totdk = np.zeros(max(n, 1), dtype=np.float64)
        o, ptrs = _trv_outputs(tables)
        _check(load_library().mfx_debug_score_paths_trv(self.h, *(paths.args() + tables.args() + [1 if need_dk else 0, C.c_void_p(numM.ctypes.data),
                                                                                                     C.c_void_p(totdk.ctypes.data)] + ptrs)))
        o = _trv_trim(o, tables)
        o["numM"], o["totdk"] = numM[:n], totdk[:n]
        return o

    def dump_values(self, seqs, contig, pos_begin, pos_end):
        n = pos_end - pos_begin
        r = np.zeros(max(n, 1), dtype=np.uint32)
        a = np.zeros(max(n, 1), dtype=np.uint32)
        ka, km = C.c_uint64(0), C.c_uint64(0)
        _check(load_library().mfx_dump_values(self.h, seqs.h, contig, pos_begin, pos_end,
                                              r.ctypes.data_as(C.POINTER(C.c_uint32)), a.ctypes.data_as(C.POINTER(C.c_uint32)),
                                              C.byref(ka), C.byref(km)))
        return r[:n], a[:n], ka.value, km.value

    def dump_contig(self, seqs, contig, name, path, append=False):
        ka, km = C.c_uint64(0), C.c_uint64(0)
        _check(load_library().mfx_dump_contig(self.h, seqs.h, contig, name.encode(), path.encode(), 1 if append else 0,
                                              C.byref(ka), C.byref(km)))
        return ka.value, km.value

    def track(self, seqs, window):
        """K* per window of `window` k-mer start positions of every contig, reduced on the device (mfx_track_run): a structured
        array of dtype TRACK_DTYPE, one record per window (contig by contig), and the totals kasm, kmissing"""
        L = load_library()
        if int(window) < 0 or int(window) >= 2**64:
            raise MfxError(-1, "track: the window must be an integer in [1, 2^64)")
        n = L.mfx_track_num_windows(seqs.h, int(window))
        w = np.zeros(max(n, 1), dtype=TRACK_DTYPE)
        got, ka, km = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(L.mfx_track_run(self.h, seqs.h, int(window), C.c_void_p(w.ctypes.data), n, C.byref(got), C.byref(ka), C.byref(km)))
        return w[:got.value], ka.value, km.value

    def regions(self, seqs, kstar=1.0, gap=0, min_kmers=1, times=None):
        """maximal runs of missing (readK == 0), collapsed (K* >= kstar) and expanded (K* <= -kstar) k-mers of every contig, runs of
        a class joined over at most `gap` positions and regions of fewer than min_kmers flagged k-mers dropped, made on the device
        (mfx_regions_run): a structured array of dtype REGION_DTYPE ordered by contig, start, class; the totals kasm, kmissing; and
        the number of tiles the second pass evaluated.  times: a list that receives the milliseconds of pass 1, runs / joining, pass 2"""
        L = load_library()
        o = _regions_opts(kstar, gap, min_kmers)
        h = C.c_void_p(None)
        ka, km = C.c_uint64(0), C.c_uint64(0)
        _check(L.mfx_regions_run(self.h, seqs.h, C.byref(o), C.byref(h), C.byref(ka), C.byref(km)))
        try:
            n = L.mfx_regions_count(h)
            r = np.zeros(max(n, 1), dtype=REGION_DTYPE)
            _check(L.mfx_regions_copy(h, C.c_void_p(r.ctypes.data), n))
            revisited = L.mfx_regions_tiles_revisited(h)
            if times is not None:
                ms = (C.c_double * 3)()
                L.mfx_diag_regions_times(h, ms)
                times[:] = list(ms)
        finally:
            L.mfx_regions_free(h)
        return r[:n], ka.value, km.value, revisited

    def phase(self, seqs, switches=100, range_=20000, times=None):
        """hap-mer phase blocks of every contig (mfx_phase_run): the index holds set A on its read side and set B on its assembly side;
        a position whose k-mer is in exactly one set is a marker, runs of at most `switches` markers within `range_` bases are short
        and do not break a block.  Returns (blocks, contig_counts): a structured array of dtype PHASE_DTYPE ordered by contig, start,
        and a uint64 array [ncontigs, 4] of valid k-mers, A markers, B markers and shared k-mers.  The K* parameters are not read.
        times: a list that receives the milliseconds of pass 1 and of runs / blocks"""
        L = load_library()
        o = _phase_opts(switches, range_)
        h = C.c_void_p(None)
        _check(L.mfx_phase_run(self.h, seqs.h, C.byref(o), C.byref(h)))
        try:
            n = L.mfx_phase_count(h)
            r = np.zeros(max(n, 1), dtype=PHASE_DTYPE)
            _check(L.mfx_phase_copy(h, C.c_void_p(r.ctypes.data), n))
            nc = seqs.ncontigs
            cc = np.zeros((max(nc, 1), 4), dtype=np.uint64)
            _check(L.mfx_phase_contig_counts(h, C.c_void_p(cc.ctypes.data), nc))
            if times is not None:
                ms = (C.c_double * 2)()
                L.mfx_diag_phase_times(h, ms)
                times[:] = list(ms)
        finally:
            L.mfx_phase_free(h)
        return r[:n], cc[:nc]

    def bin_reads(self, reads, batch_bases=0, with_stats=False, chunk=4096):
        """per-read hap-mer counts (mfx_bin_*): the index holds set A on its read side and set B on its assembly side, as for phase().
        Returns a uint32 array [n, 4] of valid k-mers, k-mers in A only, in B only and in both, one row per read in input order; with
        with_stats also the statistics of the run as a dict.  The K* parameters are not read."""
        reads = list(reads)
        b = Binner(self, batch_bases)
        out = np.zeros((len(reads), 4), dtype=np.uint32)
        got = 0
        try:
            for o in range(0, len(reads), chunk):
                b.add(reads[o:o + chunk])
                r = b.take(b.ready())
                out[got:got + len(r)] = r
                got += len(r)
            b.flush()
            r = b.take(b.ready())
            out[got:got + len(r)] = r
            got += len(r)
            st = b.end()
        finally:
            b.close()
        if got != len(reads):
            raise MfxError(-3, "bin_reads: %d records in, %d out" % (len(reads), got))
        return (out, st) if with_stats else out

    def variants(self, mode, vcf_path, names, contigs, out_path, comb=15, nosplit=False, debug_path=None, log_path=None):
        """-filter/-polish/-better/-strict/-loose over all contigs; returns clusters evaluated"""
        n = len(contigs)
        nm = (C.c_char_p * n)(*[x.encode() for x in names])
        arr = (C.c_char_p * n)(*contigs)
        lens = np.array([len(c) for c in contigs], dtype=np.uint64)
        o = _VarOpts(VARIANT_MODES[mode], comb, 1 if nosplit else 0, debug_path.encode() if debug_path else None)
        ncl = C.c_uint64(0)
        _check(load_library().mfx_variants_run(self.h, vcf_path.encode(), nm, arr, lens.ctypes.data_as(C.POINTER(C.c_uint64)), n,
                                               C.byref(o), out_path.encode(), log_path.encode() if log_path else None, C.byref(ncl)))
        return ncl.value

    def variants_loaded(self, mode, vcf, names, contigs, out_path, comb=15, nosplit=False, debug_path=None, log_path=None):
        """the same on a VCF read ahead of the run (LoadedVcf: mfx_vcf_load, host work only); the handle serves one run"""
        n = len(contigs)
        nm = (C.c_char_p * n)(*[x.encode() for x in names])
        arr = (C.c_char_p * n)(*contigs)
        lens = np.array([len(c) for c in contigs], dtype=np.uint64)
        o = _VarOpts(VARIANT_MODES[mode], comb, 1 if nosplit else 0, debug_path.encode() if debug_path else None)
        ncl = C.c_uint64(0)
        _check(load_library().mfx_variants_run_vcf(self.h, vcf.h, nm, arr, lens.ctypes.data_as(C.POINTER(C.c_uint64)), n,
                                                   C.byref(o), out_path.encode(), log_path.encode() if log_path else None, C.byref(ncl)))
        return ncl.value

    def completeness_pieces(self):
        t = np.zeros(64)
        u = np.zeros(64)
        _check(load_library().mfx_completeness_pieces(self.h, t.ctypes.data_as(C.POINTER(C.c_double)), u.ctypes.data_as(C.POINTER(C.c_double))))
        return t, u

    def completeness(self):
        t, u = C.c_double(), C.c_double()
        _check(load_library().mfx_completeness(self.h, C.byref(t), C.byref(u)))
        return t.value, u.value

    def close(self):
        if getattr(self, "h", None):
            load_library().mfx_eval_free(self.h)
            self.h = None

    def __del__(self):
        self.close()
