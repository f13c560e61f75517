"""ctypes binding of include/phi_amd.h (libphi_amd.so).

The library is the product: if it is missing or cannot be loaded this module raises, it never
falls back to a CPU implementation.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PHI_AMD_LIB") or os.path.join(_HERE, "libphi_amd.so")   # (PHI_AMD_LIB: an experimental build)

PHI_OK = 0
PHI_ERR_INVALID, PHI_ERR_NOMEM, PHI_ERR_DEVICE, PHI_ERR_STATE = -1, -2, -3, -4
PHI_ERR_UNSUPPORTED, PHI_ERR_WALK, PHI_ERR_OVERFLOW = -5, -6, -7
PHI_FLAG_QCLP, PHI_FLAG_MIXED = 1, 2
PHI_COMM_ID_BYTES = 128

# every symbol include/phi_amd.h declares
SYMBOLS = [
    "phi_strerror", "phi_last_error", "phi_ctx_create", "phi_ctx_destroy", "phi_set_stream", "phi_set_params",
    "phi_set_graph", "phi_add_reads", "phi_add_reads_device", "phi_reset_reads", "phi_reads_stats", "phi_hits_buffer", "phi_read_table",
    "phi_spectrum_export", "phi_spectrum_import", "phi_spectrum_set_size", "phi_solve", "phi_path_sequence",
    "phi_sketch", "phi_walk_minimizers", "phi_walk_sharing", "phi_kept_anchors", "phi_prof_enable", "phi_prof_read",
    "phi_host_register", "phi_host_unregister", "phi_set_solve_budget", "phi_device_synchronize", "phi_walk_text_upload", "phi_walk_text_resolve", "phi_walk_entries",
    "phi_index_stats", "phi_solve_stats", "phi_dp_probe", "phi_comm_unique_id", "phi_comm_init", "phi_comm_info", "phi_comm_allreduce_hits", "phi_comm_exchange", "phi_comm_destroy",
    "phi_reads_text_begin", "phi_add_reads_text", "phi_reads_text_end", "phi_reads_text_detach_carry", "phi_reads_text_last_batch",
    "phi_text_park_create", "phi_text_park_pin", "phi_text_park_add", "phi_text_park_add_async", "phi_text_park_wait", "phi_text_park_bytes", "phi_text_park_fetch", "phi_text_park_release", "phi_text_park_destroy",
    "phi_add_reads_text_parked",
    "phi_peers_create", "phi_peers_join", "phi_peers_allreduce_hits", "phi_peers_exchange", "phi_peers_destroy",
    "phi_ipc_unique_id", "phi_ipc_init", "phi_ipc_info", "phi_ipc_allreduce_hits", "phi_ipc_flush", "phi_ipc_exchange", "phi_ipc_check", "phi_ipc_destroy",
    "phi_edit_distances", "phi_edit_alignments",
    "phi_inflate", "phi_inflate_alloc", "phi_inflate_free", "phi_gzip_header", "phi_crc32_combine",
    "phi_text_park_gzip_begin", "phi_text_park_gzip_add", "phi_text_park_gzip_end",
    "phi_gfa_gzip_split", "phi_gfa_gzip_free",
    "phi_set_graph_chopped", "phi_chop_origin", "phi_chop_stats",
    "phi_vcf_genotypes", "phi_vcf_walks", "phi_vcf_stats",
    "phi_reads_collect_begin", "phi_reads_collect_end", "phi_reads_collect_release", "phi_ladder_plan", "phi_ladder_advance", "phi_ladder_band",
    "phi_set_graph_panel", "phi_panel_origin", "phi_panel_walks", "phi_panel_stats", "phi_panel_release",
    "phi_scout_graph", "phi_scout_scores", "phi_scout_choose", "phi_reads_collect_score", "phi_vcf_walks_wide",
    "phi_prefix_sums",
    "phi_reads_bam_begin", "phi_add_reads_bam", "phi_add_reads_bam_parked", "phi_reads_bam_end", "phi_reads_bam_last_batch",
    "phi_calls_path", "phi_calls_walk", "phi_calls_stats", "phi_calls_support", "phi_calls_support_stats",
    "phi_deflate_bgzf_bound", "phi_deflate_bgzf", "phi_deflate_bgzf_alloc", "phi_deflate_free",
    "phi_deflate_bgzf_indexed", "phi_vcf_region_filter", "phi_vcf_region_free",
]
PHI_PANEL_RETAIN = 1
PHI_PANEL_KEEP_READS = 2
PHI_SCOUT_MAX_WALKS = 65535
PHI_LADDER_MAX_LEVELS = 16
PHI_INFLATE_NO_FINDER = 1
PHI_INFLATE_CHUNK_DEFAULT = 64 << 10          # include/phi_amd.h
PHI_BGZF_BLOCK = 65280
PHI_DEFLATE_NO_MATCH = 1
PHI_DEFLATE_NO_EOF = 2
PHI_DEFLATE_BATCH_DEFAULT = 512
PHI_BGZF_INDEX_GZI = 1
PHI_BGZF_INDEX_TBI_VCF = 2


class PhiIndexInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_entries", "walk_bases", "n_classes", "class_bases", "n_class_records",
                                         "n_walk_minimizers", "n_distinct_minimizers")] + [("sketch_gpu_ms", C.c_double)]


class PhiSolveInfo(C.Structure):
    _fields_ = [("n_dp_anchors", C.c_int64), ("n_events", C.c_int64), ("n_steps", C.c_int32), ("n_blocks", C.c_int32),
                ("dp_mode", C.c_int32), ("max_classes", C.c_int32), ("mean_classes", C.c_double)]


class PhiDpProbeInfo(C.Structure):
    _fields_ = [("dp_mode", C.c_int32), ("n_blocks", C.c_int32), ("blk_ring", C.c_int32), ("blk_max_len", C.c_int32),
                ("max_classes", C.c_int32), ("retries", C.c_uint32), ("retries_since_solve", C.c_uint32)]


PHI_DP_RETRY_HALVE_CLASS_TARGET, PHI_DP_RETRY_NO_SMALL_BLOCKS, PHI_DP_RETRY_GIVE_UP_BLOCKS, PHI_DP_RETRY_DENSE = 1, 2, 4, 8


class PhiChopInfo(C.Structure):
    _fields_ = [("n_vtx_in", C.c_int64), ("n_vtx_out", C.c_int64), ("n_entries_in", C.c_int64), ("n_entries_out", C.c_int64),
                ("max_len", C.c_int32), ("expand_gpu_ms", C.c_double)]


class PhiPanelInfo(C.Structure):
    _fields_ = [("n_walks_in", C.c_int32), ("n_walks_out", C.c_int32), ("n_vtx_in", C.c_int64), ("n_vtx_out", C.c_int64),
                ("n_edges_in", C.c_int64), ("n_edges_out", C.c_int64), ("n_entries_in", C.c_int64), ("n_entries_out", C.c_int64),
                ("mark_gpu_ms", C.c_double), ("scan_gpu_ms", C.c_double), ("remap_gpu_ms", C.c_double),
                ("reduce_host_s", C.c_double), ("kahn_host_s", C.c_double)]


class PhiScoutInfo(C.Structure):
    _fields_ = [("n_blocks", C.c_int32), ("n_walks", C.c_int32), ("n_classes_flagged", C.c_int64), ("n_nonzero", C.c_int64),
                ("record_gpu_ms", C.c_double), ("class_gpu_ms", C.c_double), ("entry_gpu_ms", C.c_double), ("walk_sum_gpu_ms", C.c_double)]


class PhiVcfInfo(C.Structure):
    _fields_ = [("text_bytes", C.c_int64), ("n_records", C.c_int64), ("n_samples", C.c_int32), ("n_flagged", C.c_int64),
                ("n_units", C.c_int64), ("n_entries", C.c_int64), ("genotype_gpu_ms", C.c_double), ("walks_gpu_ms", C.c_double)]


class PhiLadderInfo(C.Structure):
    _fields_ = [("n_levels", C.c_int32), ("one_length", C.c_int32), ("n_reads", C.c_int64), ("n_bases", C.c_int64),
                ("n_kept_reads", C.c_int64), ("n_kept_bases", C.c_int64),
                ("band_reads", C.c_int64 * PHI_LADDER_MAX_LEVELS), ("band_bases", C.c_int64 * PHI_LADDER_MAX_LEVELS),
                ("threshold", C.c_uint64 * PHI_LADDER_MAX_LEVELS),
                ("count_gpu_ms", C.c_double), ("scan_gpu_ms", C.c_double), ("scatter_gpu_ms", C.c_double), ("copy_gpu_ms", C.c_double)]


class PhiBamInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_records", "n_kept", "n_secondary_supplementary", "n_empty", "n_reverse", "n_bases", "header_bytes",
                                         "tiles", "tiles_confirmed", "tiles_rewalked", "batches", "batches_without_offsets")] + [
        ("n_ref", C.c_int32), ("one_length", C.c_int32)]


class PhiCalls(C.Structure):
    _fields_ = [("n_calls", C.c_int64), ("pos", C.POINTER(C.c_int64)), ("ref_off", C.POINTER(C.c_int64)), ("alt_off", C.POINTER(C.c_int64)),
                ("ref_bytes", C.c_void_p), ("alt_bytes", C.c_void_p), ("anchor", C.POINTER(C.c_int32)),
                ("n_shared", C.c_int64), ("n_query", C.c_int64), ("n_ref", C.c_int64),
                ("ref_span", C.c_int64 * 2), ("query_span", C.c_int64 * 2), ("gpu_ms", C.c_double)]


class PhiCallSupport(C.Structure):
    _fields_ = [("n_calls", C.c_int64)] + [(n, C.POINTER(C.c_int32)) for n in ("alt_hit", "alt_n", "ref_hit", "ref_n")] + [
        (n, C.c_int64) for n in ("alt_hit_total", "alt_n_total", "ref_hit_total", "ref_n_total", "n_items")] + [("gpu_ms", C.c_double)]


class PhiCallsSupportInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_calls", "n_items", "n_visited", "n_records", "n_witnesses", "bytes_moved")] + [("gpu_ms", C.c_double)]


class PhiCallsInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_query", "n_ref", "n_shared", "n_pairs", "n_calls", "ref_bytes", "alt_bytes", "ref_bases", "query_bases", "bytes_moved")] + [
        (n, C.c_double) for n in ("table_gpu_ms", "shared_gpu_ms", "pairs_gpu_ms", "fill_gpu_ms", "gpu_ms")]


class PhiResult(C.Structure):
    _fields_ = [
        ("objective", C.c_int64), ("upper_bound", C.c_int64), ("optimal", C.c_int32), ("n_dp_runs", C.c_int32),
        ("n_covered", C.c_int64),
        ("n_path", C.c_int64), ("path_vtx", C.POINTER(C.c_int32)), ("path_hap", C.POINTER(C.c_int32)),
        ("recombination_count", C.c_int32), ("n_switches", C.c_int32), ("hap_len", C.c_int64),
        ("n_walks", C.c_int32), ("n_minimizers", C.POINTER(C.c_int64)), ("n_anchors", C.POINTER(C.c_int64)),
        ("spectrum_size", C.c_int64), ("filtered", C.c_int64), ("retained", C.c_int64), ("n_in_model", C.c_int64),
    ]


class PhiInflateInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("in_bytes", "out_bytes", "members", "chunks", "confirmed", "redecoded", "marker_bytes")] + [
        ("device_ms", C.c_double), ("detail", C.c_char * 192)]


class PhiDeflateInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("in_bytes", "out_bytes", "blocks", "stored_blocks", "matches", "match_bytes")] + [
        ("device_ms", C.c_double), ("detail", C.c_char * 192)]


class PhiVcfRegionInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("members", "gz_bytes", "text_bytes", "lines_seen", "lines_kept", "batches", "reinflated_members")] + [
        ("inflate_ms", C.c_double), ("filter_ms", C.c_double), ("detail", C.c_char * 192)]


class PhiBgzfIndexInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("records", "meta_lines", "contigs", "bins", "chunks", "windows", "index_bytes")] + [
        ("device_ms", C.c_double), ("detail", C.c_char * 192)]


class PhiGfaGzipInfo(C.Structure):
    _fields_ = [("text_bytes", C.c_int64), ("host_bytes", C.c_int64), ("walk_bytes", C.c_int64), ("n_walks", C.c_int32),
                ("inflate", PhiInflateInfo)]


_lib = None


def load():
    """Load libphi_amd.so and declare the prototypes.  Raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -m phi_amd.build` "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.phi_strerror.restype = C.c_char_p
    L.phi_strerror.argtypes = [C.c_int]
    L.phi_last_error.restype = C.c_char_p
    L.phi_last_error.argtypes = [vp]
    L.phi_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.phi_ctx_destroy.restype = None
    L.phi_ctx_destroy.argtypes = [vp]
    L.phi_set_stream.argtypes = [vp, vp]
    L.phi_set_params.argtypes = [vp, i32, i32, C.c_float, i32, C.c_uint32]
    L.phi_set_graph.argtypes = [vp, i32, vp, vp, vp, vp, i32, vp, vp, vp]
    L.phi_set_graph_chopped.argtypes = [vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp]
    L.phi_chop_origin.argtypes = [vp, vp, i64, vp, vp]
    L.phi_chop_stats.argtypes = [vp, C.POINTER(PhiChopInfo)]
    L.phi_set_graph_panel.argtypes = [vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, i32, C.c_uint32, vp]
    L.phi_panel_origin.argtypes = [vp, vp, i64, vp]
    L.phi_panel_walks.argtypes = [vp, vp, i32, C.POINTER(i32)]
    L.phi_panel_stats.argtypes = [vp, C.POINTER(PhiPanelInfo)]
    L.phi_panel_release.argtypes = [vp]
    L.phi_scout_graph.argtypes = [vp, i32, vp, vp, vp, vp, i32, vp, vp, vp]
    L.phi_scout_scores.argtypes = [vp, i32, vp, C.POINTER(PhiScoutInfo)]
    L.phi_scout_choose.argtypes = [vp, vp, i32, vp, vp]
    L.phi_reads_collect_score.argtypes = [vp]
    L.phi_vcf_walks_wide.argtypes = [vp, vp, i64, vp, vp, i64, vp, i32, vp]
    L.phi_vcf_genotypes.argtypes = [vp, vp, i64, vp, vp, i64, i32, vp, vp, vp]
    L.phi_vcf_walks.argtypes = [vp, vp, i64, vp, vp, i64, vp, i32, vp]
    L.phi_vcf_stats.argtypes = [vp, C.POINTER(PhiVcfInfo)]
    L.phi_reads_collect_begin.argtypes = [vp, i64]
    L.phi_reads_collect_end.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.phi_reads_collect_release.argtypes = [vp]
    L.phi_ladder_plan.argtypes = [vp, C.c_uint64, C.POINTER(C.c_double), i32, C.POINTER(PhiLadderInfo)]
    L.phi_ladder_advance.argtypes = [vp, i32]
    L.phi_ladder_band.argtypes = [vp, i32, vp, i64, C.POINTER(i64), vp, i64, vp, C.POINTER(i64)]
    L.phi_add_reads.argtypes = [vp, vp, vp, i64]
    L.phi_add_reads_device.argtypes = [vp, vp, vp, i64, i64]
    L.phi_reset_reads.argtypes = [vp]
    L.phi_reads_text_begin.argtypes = [vp, i64]
    L.phi_add_reads_text.argtypes = [vp, vp, i64, C.POINTER(i32)]
    L.phi_reads_text_end.argtypes = [vp, C.POINTER(vp), C.POINTER(i64), C.POINTER(i64)]
    L.phi_reads_text_detach_carry.argtypes = [vp, C.POINTER(vp), C.POINTER(i64)]
    L.phi_reads_text_last_batch.argtypes = [vp, vp, i64, vp, i64, C.POINTER(i64), C.POINTER(i64)]
    L.phi_text_park_create.argtypes = [i32, C.POINTER(vp)]
    L.phi_text_park_pin.argtypes = [vp, vp, C.c_size_t]
    L.phi_text_park_add.argtypes = [vp, vp, i64, C.POINTER(i32)]
    L.phi_text_park_add_async.argtypes = [vp, vp, i64, C.POINTER(i32)]
    L.phi_text_park_wait.argtypes = [vp, i32]
    L.phi_text_park_bytes.argtypes = [vp, i32]
    L.phi_text_park_bytes.restype = i64
    L.phi_text_park_fetch.argtypes = [vp, i32, vp, i64]
    L.phi_text_park_release.argtypes = [vp, i32]
    L.phi_text_park_destroy.argtypes = [vp]
    L.phi_text_park_destroy.restype = None
    L.phi_add_reads_text_parked.argtypes = [vp, vp, i32, C.POINTER(i32)]
    L.phi_reads_bam_begin.argtypes = [vp, i64, i64]
    L.phi_add_reads_bam.argtypes = [vp, vp, i64]
    L.phi_add_reads_bam_parked.argtypes = [vp, vp, i32]
    L.phi_reads_bam_end.argtypes = [vp, C.POINTER(PhiBamInfo)]
    L.phi_reads_bam_last_batch.argtypes = [vp, vp, i64, vp, i64, C.POINTER(i64), C.POINTER(i64)]
    L.phi_calls_path.argtypes = [vp, i32, C.POINTER(PhiCalls)]
    L.phi_calls_walk.argtypes = [vp, i32, i32, C.POINTER(PhiCalls)]
    L.phi_calls_stats.argtypes = [vp, C.POINTER(PhiCallsInfo)]
    L.phi_calls_support.argtypes = [vp, C.POINTER(PhiCallSupport)]
    L.phi_calls_support_stats.argtypes = [vp, C.POINTER(PhiCallsSupportInfo)]
    L.phi_reads_stats.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.phi_hits_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(i64)]
    L.phi_read_table.argtypes = [vp, C.POINTER(vp), C.POINTER(i64)]
    L.phi_spectrum_export.argtypes = [vp, C.POINTER(vp), C.POINTER(i64)]
    L.phi_spectrum_import.argtypes = [vp, vp, i64]
    L.phi_spectrum_set_size.argtypes = [vp, i64]
    L.phi_solve.argtypes = [vp, C.POINTER(PhiResult)]
    L.phi_set_solve_budget.argtypes = [vp, i64]
    L.phi_index_stats.argtypes = [vp, C.POINTER(PhiIndexInfo)]
    L.phi_solve_stats.argtypes = [vp, C.POINTER(PhiSolveInfo)]
    L.phi_dp_probe.argtypes = [vp, vp, i64, vp, C.POINTER(i64), C.POINTER(i32), vp, vp, vp, i64, C.POINTER(i64), C.POINTER(PhiDpProbeInfo)]
    L.phi_comm_unique_id.argtypes = [vp, C.c_size_t]
    L.phi_comm_init.argtypes = [vp, vp, i32, i32]
    L.phi_comm_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.phi_comm_allreduce_hits.argtypes = [vp]
    L.phi_comm_exchange.argtypes = [vp]
    L.phi_comm_destroy.argtypes = [vp]
    L.phi_peers_create.argtypes = [i32, C.POINTER(vp)]
    L.phi_peers_join.argtypes = [vp, vp, i32]
    L.phi_peers_allreduce_hits.argtypes = [vp]
    L.phi_peers_exchange.argtypes = [vp]
    L.phi_peers_destroy.argtypes = [vp]
    L.phi_ipc_unique_id.argtypes = [vp, C.c_size_t]
    L.phi_ipc_init.argtypes = [vp, C.c_char_p, i32, i32]
    L.phi_ipc_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.phi_ipc_allreduce_hits.argtypes = [vp]
    L.phi_ipc_exchange.argtypes = [vp]
    L.phi_ipc_flush.argtypes = [vp]
    L.phi_ipc_check.argtypes = [vp]
    L.phi_ipc_destroy.argtypes = [vp]
    L.phi_path_sequence.argtypes = [vp, vp, i64]
    L.phi_sketch.argtypes = [vp, vp, vp, i64, i32, i32, vp, vp, vp, i64, C.POINTER(i64)]
    L.phi_walk_minimizers.argtypes = [vp, i32, vp, vp, i64, C.POINTER(i64)]
    L.phi_walk_sharing.argtypes = [vp, vp, i32, C.POINTER(i64)]
    L.phi_kept_anchors.argtypes = [vp, vp, vp, vp, vp, i64, C.POINTER(i64)]
    L.phi_prof_enable.argtypes = [vp, C.c_int]
    L.phi_host_register.argtypes = [vp, vp, C.c_size_t]
    L.phi_host_unregister.argtypes = [vp, vp]
    L.phi_prof_read.argtypes = [vp, C.POINTER(i64), C.POINTER(C.c_double), C.POINTER(i64)]
    L.phi_device_synchronize.argtypes = [vp]
    L.phi_prefix_sums.argtypes = [vp, i32, vp, i64, vp]
    L.phi_walk_text_upload.argtypes = [vp, vp, i32]
    L.phi_walk_text_resolve.argtypes = [vp, C.c_char_p, i32, vp, i64, i32, vp, C.POINTER(C.c_uint32)]
    L.phi_walk_entries.argtypes = [vp, vp, i64, C.POINTER(i64)]
    L.phi_edit_distances.argtypes = [vp, vp, vp, vp, vp, i64, i64, vp]
    L.phi_edit_alignments.argtypes = [vp, vp, vp, vp, vp, i64, vp, vp, vp, vp]
    L.phi_inflate.argtypes = [i32, vp, i64, vp, i64, i64, i32, C.POINTER(i64), C.POINTER(PhiInflateInfo)]
    L.phi_inflate_alloc.argtypes = [i32, vp, i64, i64, i32, C.POINTER(vp), C.POINTER(i64), C.POINTER(PhiInflateInfo)]
    L.phi_inflate_free.argtypes = [vp]
    L.phi_inflate_free.restype = None
    L.phi_deflate_bgzf_bound.argtypes = [i64]
    L.phi_deflate_bgzf_bound.restype = i64
    L.phi_deflate_bgzf.argtypes = [i32, vp, i64, vp, i64, i32, C.POINTER(i64), C.POINTER(PhiDeflateInfo)]
    L.phi_deflate_bgzf_alloc.argtypes = [i32, vp, i64, i32, C.POINTER(vp), C.POINTER(i64), C.POINTER(PhiDeflateInfo)]
    L.phi_deflate_bgzf_indexed.argtypes = [i32, vp, i64, i32, i32, C.POINTER(vp), C.POINTER(i64), C.POINTER(vp), C.POINTER(i64),
                                           C.POINTER(PhiDeflateInfo), C.POINTER(PhiBgzfIndexInfo)]
    L.phi_deflate_free.argtypes = [vp]
    L.phi_deflate_free.restype = None
    L.phi_vcf_region_filter.argtypes = [i32, vp, i64, vp, i32, C.c_char_p, i64, i64, C.POINTER(vp), C.POINTER(i64), C.POINTER(PhiVcfRegionInfo)]
    L.phi_vcf_region_free.argtypes = [vp]
    L.phi_vcf_region_free.restype = None
    L.phi_text_park_gzip_begin.argtypes = [vp, i64]
    L.phi_text_park_gzip_add.argtypes = [vp, vp, i64]
    L.phi_text_park_gzip_end.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(PhiInflateInfo)]
    L.phi_gzip_header.argtypes = [vp, i64, i64, C.POINTER(i64)]
    L.phi_crc32_combine.argtypes = [C.c_uint32, C.c_uint32, i64]
    L.phi_crc32_combine.restype = C.c_uint32
    L.phi_gfa_gzip_split.argtypes = [vp, vp, i64, i64, C.POINTER(vp), C.POINTER(i64), C.POINTER(PhiGfaGzipInfo)]
    L.phi_gfa_gzip_free.argtypes = [vp]
    L.phi_gfa_gzip_free.restype = None
    for name in SYMBOLS:
        f = getattr(L, name)          # AttributeError here = the library does not export the ABI
        if f.restype is C.c_int and name not in ("phi_strerror", "phi_last_error", "phi_ctx_destroy", "phi_crc32_combine", "phi_inflate_free", "phi_gfa_gzip_free", "phi_deflate_bgzf_bound", "phi_deflate_free"):
            f.restype = C.c_int
    _lib = L
    return L
