"""merfin_amd -- MI355X-native k-mer multiplicity evaluator (merfin's -hist /
-dump / -completeness evaluation path on gfx950).

This package is a thin ctypes binding of the C ABI in include/merfin_amd.h
(libmerfin_amd.so, hand-written HIP).  It exists for the parity tests and
bench.py; the product host program is the C++ `merfin` CLI in merfin_amd/cli.
There is no CPU fallback: importing works anywhere, but creating an index
without the HIP library or without a GPU raises.
"""
from .binding import (  # noqa: F401
    MfxError, E_NONCANON, Index, Sequences, Evaluator, Router, HistResult, KParams,
    lib_path, load_library, device_count, device_warm, getK, getKmetric, histoQV, hist_words, result_from_counts,
    TILE, db_probe, db_write_flat, db_convert, db_merge, db_merge_except, db_merge_plan, db_join_completeness, db_join_spectrum, db_join_grain, db_join_host, PinnedBuffer, Comm, hist_multi, hist_sharded, load_db_multi, dump_values_sharded, dump_contig_sharded, variants_sharded, pack_bases, gather_rate, stream_rates, hist_parts, LoadedVcf, hist_streamed_multi, stream_share, DbStage, DbWriter, ReadsStore, db_convert_placed, db_place_keys, db_write_flat_placed,
    track_write, TRACK_DTYPE, regions_write, regions_from_planes_host, phase_write, phase_from_planes_host, PHASE_DTYPE, REGION_DTYPE, REGION_CLASSES, WORKLIST_DTYPE, spectrum_peak, spectrum_write, E_NODATA, db_trio, db_trio_hist, db_trio_host, db_histogram, db_histogram_write, db_diploid, db_diploid_host, diploid_write_asm, DIPLOID_CLASSES,
    Binner, bin_classify, bin_plan_host, BIN_CLASSES,
)

__all__ = ["MfxError", "E_NONCANON", "Index", "Sequences", "Evaluator", "Router", "HistResult", "KParams", "lib_path",
           "load_library", "device_count", "device_warm", "getK", "getKmetric", "histoQV", "hist_words", "result_from_counts", "TILE", "db_probe", "db_write_flat", "db_convert", "db_merge", "db_merge_except", "db_merge_plan", "db_join_completeness", "db_join_spectrum", "db_join_grain", "db_join_host",
           "PinnedBuffer", "Comm", "hist_multi", "hist_sharded", "load_db_multi", "dump_values_sharded", "dump_contig_sharded", "variants_sharded", "pack_bases", "gather_rate", "stream_rates", "hist_parts", "LoadedVcf", "hist_streamed_multi", "stream_share", "DbStage", "DbWriter", "ReadsStore", "db_convert_placed", "db_place_keys", "db_write_flat_placed", "track_write", "TRACK_DTYPE", "regions_write", "regions_from_planes_host", "phase_write", "phase_from_planes_host", "PHASE_DTYPE", "REGION_DTYPE", "REGION_CLASSES", "WORKLIST_DTYPE", "spectrum_peak", "spectrum_write", "E_NODATA", "db_trio", "db_trio_hist", "db_trio_host", "db_histogram", "db_histogram_write", "db_diploid", "db_diploid_host", "diploid_write_asm", "DIPLOID_CLASSES", "Binner", "bin_classify", "bin_plan_host", "BIN_CLASSES"]
