"""ctypes loader of libvbz_hip.so (the C ABI in include/vbz.h, include/vbz_gpu.h and include/vbz_gpu_pile.h).

The library is the product: if it is missing this module raises -- there is no Python or CPU
fallback for either stage of the codec.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# VBZ_HIP_LIB: another build of the same library (tools/ab_libs.py; the experiments build lib/libvbz_hip_x.so that carries the
# timed kernel instantiations for tools/ and the svb hand-over test aid for tests/test_gpu_handover.py)
LIB_PATH = os.environ.get("VBZ_HIP_LIB") or os.path.join(HERE, "lib", "libvbz_hip.so")
EXPERIMENTS_LIB_PATH = os.path.join(HERE, "lib", "libvbz_hip_x.so")
PLUGIN_PATH = os.path.join(HERE, "lib", "libvbz_hdf_plugin.so")

VBZ_ZSTD_ERROR = 0xFFFFFFFF
VBZ_INPUT_SIZE_ERROR = 0xFFFFFFFE
VBZ_INTEGER_SIZE_ERROR = 0xFFFFFFFD
VBZ_DESTINATION_SIZE_ERROR = 0xFFFFFFFC
VBZ_STREAMVBYTE_STREAM_ERROR = 0xFFFFFFFB
VBZ_VERSION_ERROR = 0xFFFFFFFA
VBZ_OUT_OF_MEMORY_ERROR = 0xFFFFFFF9
VBZ_DEVICE_ERROR = 0xFFFFFFF8  # vbz_gpu.h results only
VBZ_FIRST_ERROR = VBZ_OUT_OF_MEMORY_ERROR  # the reference's value (vbz/vbz.h:22)


class CompressionOptions(ctypes.Structure):
    """struct CompressionOptions of include/vbz.h (reference vbz/vbz.h:29-53), 16 bytes."""

    _fields_ = [
        ("perform_delta_zig_zag", ctypes.c_bool),
        ("integer_size", ctypes.c_uint),
        ("zstd_compression_level", ctypes.c_uint),
        ("vbz_version", ctypes.c_uint),
    ]


class GpuBatch(ctypes.Structure):
    """struct vbz_gpu_batch of include/vbz_gpu.h."""

    _fields_ = [
        ("n_reads", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("src", ctypes.c_void_p),
        ("src_off", ctypes.c_void_p),
        ("src_size", ctypes.c_void_p),
        ("src_bytes", ctypes.c_uint64),
        ("dst", ctypes.c_void_p),
        ("dst_off", ctypes.c_void_p),
        ("dst_cap", ctypes.c_void_p),
        ("dst_bytes", ctypes.c_uint64),
        ("result", ctypes.c_void_p),
    ]


VBZ_GPU_SIGNAL_F32 = 1
VBZ_GPU_SIGNAL_F16 = 2
VBZ_GPU_SIGNAL_BF16 = 3


class GpuSignalFormat(ctypes.Structure):
    """struct vbz_gpu_signal_format of include/vbz_gpu.h."""

    _fields_ = [
        ("out_type", ctypes.c_uint32),
        ("is_signed", ctypes.c_uint32),
        ("offset", ctypes.c_void_p),
        ("scale", ctypes.c_void_p),
    ]


VBZ_GPU_CHUNK_PAD = 0
VBZ_GPU_CHUNK_END = 1


class GpuChunking(ctypes.Structure):
    """struct vbz_gpu_chunking of include/vbz_gpu.h (24 bytes)."""

    _fields_ = [
        ("chunk_len", ctypes.c_uint32),
        ("step", ctypes.c_uint32),
        ("mode", ctypes.c_uint32),
        ("end_align", ctypes.c_uint32),
        ("pad", ctypes.c_float),
        ("reserved", ctypes.c_uint32),
    ]


VBZ_GPU_NORM_MED_MAD = 1
VBZ_GPU_NORM_QUANTILE = 2
VBZ_GPU_RANGE_STATS_RANGE = 0   # statistics of the range's samples
VBZ_GPU_RANGE_STATS_READ = 1    # statistics of the whole read

VBZ_GPU_VERSION_POD5 = 0x35444F50   # CompressionOptions.vbz_version of POD5 signal rows (svb16 + zstd; the batched API only)


class GpuPod5Reads(ctypes.Structure):
    """struct vbz_gpu_pod5_reads of include/vbz_gpu.h (24 bytes)."""

    _fields_ = [
        ("n_reads", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("first_row", ctypes.c_void_p),
        ("read_result", ctypes.c_void_p),
    ]


class GpuNormalization(ctypes.Structure):
    """struct vbz_gpu_normalization of include/vbz_gpu.h (32 bytes)."""

    _fields_ = [
        ("method", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("quantile_a", ctypes.c_float),
        ("quantile_b", ctypes.c_float),
        ("shift_mul", ctypes.c_float),
        ("scale_mul", ctypes.c_float),
        ("shift_min", ctypes.c_float),
        ("scale_min", ctypes.c_float),
    ]


class GpuSampleRanges(ctypes.Structure):
    """struct vbz_gpu_sample_ranges of include/vbz_gpu.h (24 bytes)."""

    _fields_ = [
        ("begin", ctypes.c_void_p),
        ("end", ctypes.c_void_p),
        ("stats", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


class GpuWindows(ctypes.Structure):
    """struct vbz_gpu_windows of include/vbz_gpu.h (40 bytes)."""

    _fields_ = [
        ("window_len", ctypes.c_uint32),
        ("pad", ctypes.c_float),
        ("window_rows", ctypes.c_uint64),
        ("window_first", ctypes.c_void_p),
        ("start", ctypes.c_void_p),
        ("flags", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


class GpuEvents(ctypes.Structure):
    """struct vbz_gpu_events of include/vbz_gpu.h (32 bytes)."""

    _fields_ = [
        ("event_rows", ctypes.c_uint64),
        ("event_first", ctypes.c_void_p),
        ("start", ctypes.c_void_p),
        ("flags", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


class GpuEvent(ctypes.Structure):
    """struct vbz_gpu_event of include/vbz_gpu.h (16 bytes): one row of the event arena."""

    _fields_ = [
        ("mean", ctypes.c_float),
        ("sd", ctypes.c_float),
        ("n", ctypes.c_uint32),
        ("zero", ctypes.c_uint32),
    ]


class GpuEventMoments(ctypes.Structure):
    """struct vbz_gpu_event_moments of include/vbz_gpu.h (16 bytes): one row's exact sums."""

    _fields_ = [
        ("sum", ctypes.c_int64),
        ("sumsq", ctypes.c_uint64),
    ]


VBZ_GPU_TRIM_REJECT_AT_END = 1   # vbz_gpu_trim.flags: a trim whose window ends at the end of the samples looked at is rejected


class GpuTrim(ctypes.Structure):
    """struct vbz_gpu_trim of include/vbz_gpu.h (32 bytes)."""

    _fields_ = [
        ("window", ctypes.c_uint32),
        ("min_elements", ctypes.c_uint32),
        ("min_trim", ctypes.c_uint32),
        ("max_samples", ctypes.c_uint32),
        ("threshold_factor", ctypes.c_float),
        ("max_fraction", ctypes.c_float),
        ("flags", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


class GpuSegmentation(ctypes.Structure):
    """struct vbz_gpu_segmentation of include/vbz_gpu.h (32 bytes)."""

    _fields_ = [
        ("short_window", ctypes.c_uint32),
        ("long_window", ctypes.c_uint32),
        ("short_threshold", ctypes.c_float),
        ("long_threshold", ctypes.c_float),
        ("radius", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("start_cap", ctypes.c_uint64),
    ]


VBZ_GPU_SPAN_ABOVE = 0
VBZ_GPU_SPAN_BELOW = 1


class GpuSpans(ctypes.Structure):
    """struct vbz_gpu_spans of include/vbz_gpu.h (40 bytes)."""

    _fields_ = [
        ("direction", ctypes.c_uint32),
        ("merge_gap", ctypes.c_uint32),
        ("min_length", ctypes.c_uint32),
        ("ignore_prefix", ctypes.c_uint32),
        ("threshold_factor", ctypes.c_float),
        ("flags", ctypes.c_uint32),
        ("level", ctypes.c_void_p),
        ("edge_cap", ctypes.c_uint64),
    ]


class GpuMatch(ctypes.Structure):
    """struct vbz_gpu_match of include/vbz_gpu.h (40 bytes)."""

    _fields_ = [
        ("query_len", ctypes.c_uint32),
        ("n_refs", ctypes.c_uint32),
        ("ref_stride", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("quant", ctypes.c_float),
        ("reserved", ctypes.c_uint32),
        ("ref", ctypes.c_void_p),
        ("ref_len", ctypes.c_void_p),
    ]


class GpuLocate(ctypes.Structure):
    """struct vbz_gpu_locate of include/vbz_gpu.h (40 bytes)."""

    _fields_ = [
        ("query_len", ctypes.c_uint32),
        ("n_targets", ctypes.c_uint32),
        ("target_stride", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("quant", ctypes.c_float),
        ("reserved", ctypes.c_uint32),
        ("target", ctypes.c_void_p),
        ("target_len", ctypes.c_void_p),
    ]


class GpuMatchHit(ctypes.Structure):
    """struct vbz_gpu_match_hit of include/vbz_gpu.h (8 bytes)."""

    _fields_ = [
        ("cost", ctypes.c_uint32),
        ("end", ctypes.c_uint32),
    ]


class GpuMatchSpan(ctypes.Structure):
    """struct vbz_gpu_match_span of include/vbz_gpu.h (16 bytes)."""

    _fields_ = [
        ("cost", ctypes.c_uint32),
        ("end", ctypes.c_uint32),
        ("start", ctypes.c_uint32),
        ("zero", ctypes.c_uint32),
    ]


class GpuMatchPair(ctypes.Structure):
    """struct vbz_gpu_match_pair of include/vbz_gpu.h (16 bytes)."""

    _fields_ = [
        ("read", ctypes.c_uint32),
        ("ref", ctypes.c_uint32),
        ("begin", ctypes.c_uint32),
        ("end", ctypes.c_uint32),
    ]


class GpuMatchPath(ctypes.Structure):
    """struct vbz_gpu_match_path of include/vbz_gpu.h (16 bytes)."""

    _fields_ = [
        ("max_width", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("reserved", ctypes.c_uint64),
    ]


class GpuMatchRow(ctypes.Structure):
    """struct vbz_gpu_match_row of include/vbz_gpu.h (8 bytes)."""

    _fields_ = [
        ("begin", ctypes.c_uint32),
        ("end", ctypes.c_uint32),
    ]


class GpuEventsQuery(ctypes.Structure):
    """struct vbz_gpu_events_query of include/vbz_gpu.h (16 bytes)."""

    _fields_ = [
        ("query_len", ctypes.c_uint32),
        ("min_n", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


class GpuLevel(ctypes.Structure):
    """struct vbz_gpu_level of include/vbz_gpu.h (32 bytes)."""

    _fields_ = [
        ("first_sample", ctypes.c_uint32),
        ("end_sample", ctypes.c_uint32),
        ("n_samples", ctypes.c_uint32),
        ("n_entries", ctypes.c_uint32),
        ("sum", ctypes.c_int64),
        ("sumsq", ctypes.c_uint64),
    ]


class GpuSquiggle(ctypes.Structure):
    """struct vbz_gpu_squiggle of include/vbz_gpu.h (48 bytes)."""

    _fields_ = [
        ("k", ctypes.c_uint32),
        ("n_seqs", ctypes.c_uint32),
        ("seq_stride", ctypes.c_uint32),
        ("target_stride", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("quant", ctypes.c_float),
        ("seq", ctypes.c_void_p),
        ("seq_len", ctypes.c_void_p),
        ("model", ctypes.c_void_p),
    ]


class GpuLevelsFit(ctypes.Structure):
    """struct vbz_gpu_levels_fit of include/vbz_gpu.h (16 bytes)."""

    _fields_ = [
        ("max_width", ctypes.c_uint32),
        ("min_samples", ctypes.c_uint32),
        ("max_entries", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
    ]


class GpuLevelFit(ctypes.Structure):
    """struct vbz_gpu_level_fit of include/vbz_gpu.h (16 bytes)."""

    _fields_ = [
        ("offset", ctypes.c_float),
        ("scale", ctypes.c_float),
        ("used", ctypes.c_uint32),
        ("ok", ctypes.c_uint32),
    ]


class GpuLevelsPile(ctypes.Structure):
    """struct vbz_gpu_levels_pile of include/vbz_gpu_pile.h (32 bytes)."""

    _fields_ = [
        ("max_width", ctypes.c_uint32),
        ("min_samples", ctypes.c_uint32),
        ("max_entries", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("fix", ctypes.c_float),
        ("reserved0", ctypes.c_uint32),
        ("reserved1", ctypes.c_uint32),
        ("reserved2", ctypes.c_uint32),
    ]


class GpuPileKmers(ctypes.Structure):
    """struct vbz_gpu_pile_kmers of include/vbz_gpu_pile.h (16 bytes)."""

    _fields_ = [
        ("k", ctypes.c_uint32),
        ("rows", ctypes.c_uint32),
        ("target_stride", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
    ]


class GpuModelUpdate(ctypes.Structure):
    """struct vbz_gpu_model_update of include/vbz_gpu_pile.h (16 bytes)."""

    _fields_ = [
        ("k", ctypes.c_uint32),
        ("min_obs", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("fix", ctypes.c_float),
    ]


SQUIGGLE_BOTH, SQUIGGLE_REVERSED = 1, 2
PILE_CLEAR, PILE_REQUIRE_OK, PILE_DIRECT = 1, 2, 4
KMER_MARK = 0xFFFFFFFF   # vbz_gpu_squiggle_kmers_batch: a masked k-mer, and at and behind target_len

C_API = [
    "vbz_is_error",
    "vbz_error_string",
    "vbz_max_compressed_size",
    "vbz_compress",
    "vbz_decompress",
    "vbz_compress_sized",
    "vbz_decompress_sized",
    "vbz_decompressed_size",
]
GPU_API = [
    "vbz_gpu_create",
    "vbz_gpu_destroy",
    "vbz_gpu_stream",
    "vbz_gpu_last_error",
    "vbz_gpu_set_trailers",
    "vbz_gpu_set_canonical",
    "vbz_gpu_set_checksum",
    "vbz_gpu_synchronize",
    "vbz_gpu_compress_batch",
    "vbz_gpu_decompress_batch",
    "vbz_gpu_decompress_signal_batch",
    "vbz_gpu_chunk_layout_batch",
    "vbz_gpu_decompress_chunks_batch",
    "vbz_gpu_signal_norm_batch",
    "vbz_gpu_decompress_signal_norm_batch",
    "vbz_gpu_decompress_chunks_norm_batch",
    "vbz_gpu_pod5_max_compressed_size",
    "vbz_gpu_pod5_read_samples_batch",
    "vbz_gpu_pod5_decompress_chunks_batch",
    "vbz_gpu_pod5_signal_norm_batch",
    "vbz_gpu_pod5_decompress_signal_norm_batch",
    "vbz_gpu_range_samples_batch",
    "vbz_gpu_decompress_chunks_range_batch",
    "vbz_gpu_signal_norm_range_batch",
    "vbz_gpu_pod5_decompress_chunks_range_batch",
    "vbz_gpu_pod5_signal_norm_range_batch",
    "vbz_gpu_signal_trim_batch",
    "vbz_gpu_pod5_signal_trim_batch",
    "vbz_gpu_decompress_windows_batch",
    "vbz_gpu_pod5_decompress_windows_batch",
    "vbz_gpu_signal_events_batch",
    "vbz_gpu_pod5_signal_events_batch",
    "vbz_gpu_signal_segment_batch",
    "vbz_gpu_pod5_signal_segment_batch",
    "vbz_gpu_signal_spans_batch",
    "vbz_gpu_pod5_signal_spans_batch",
    "vbz_gpu_match_batch",
    "vbz_gpu_signal_match_batch",
    "vbz_gpu_pod5_signal_match_batch",
    "vbz_gpu_match_span_batch",
    "vbz_gpu_signal_match_span_batch",
    "vbz_gpu_pod5_signal_match_span_batch",
    "vbz_gpu_match_best_batch",
    "vbz_gpu_match_path_batch",
    "vbz_gpu_set_match_path_cap",
    "vbz_gpu_locate_batch",
    "vbz_gpu_signal_locate_batch",
    "vbz_gpu_pod5_signal_locate_batch",
    "vbz_gpu_locate_span_batch",
    "vbz_gpu_signal_locate_span_batch",
    "vbz_gpu_pod5_signal_locate_span_batch",
    "vbz_gpu_locate_path_batch",
    "vbz_gpu_query_valid_batch",
    "vbz_gpu_events_query_batch",
    "vbz_gpu_locate_levels_batch",
    "vbz_gpu_squiggle_batch",
    "vbz_gpu_levels_fit_batch",
    "vbz_gpu_svb_compress_batch",
    "vbz_gpu_svb_decompress_batch",
    "vbz_gpu_zstd_compress_batch",
    "vbz_gpu_zstd_decompress_batch",
    "vbz_gpu_xxh64_batch",
    "vbz_gpu_pack_batch",
    "vbz_gpu_decompressed_size_batch",
    "vbz_gpu_synth_lengths",
    "vbz_gpu_synth_signal",
    "vbz_gpu_synth_u32",
    "vbz_gpu_profile_enable",
    "vbz_gpu_profile_read",
    "vbz_gpu_profile_reset",
    "vbz_gpu_decode_paths",
    "vbz_gpu_decode_literals_ahead",
    "vbz_gpu_decode_span_paths",
    "vbz_gpu_version",
]

# The pile-up across reads: the entry points of include/vbz_gpu_pile.h.  They stand in lists of their own: C_API + GPU_API and PROTOTYPES are
# held to tests/golden/prototypes.json, a recorded table no change edits; these are held to tests/golden/prototypes_pile.json.
PILE_API = [
    "vbz_gpu_levels_pile_batch",
    "vbz_gpu_squiggle_kmers_batch",
    "vbz_gpu_pile_kmers_batch",
    "vbz_gpu_model_update_batch",
]

def _prototypes():
    """name -> (restype, argtypes) of every entry of C_API + GPU_API, as include/vbz.h and include/vbz_gpu.h declare them.  A new entry is
    one row here; a family is derived from its base row below the literal rows."""
    c_int, vp, u32, u64, P = ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER
    op, bp, fp, cp, np_, rp, gp = P(CompressionOptions), P(GpuBatch), P(GpuSignalFormat), P(GpuChunking), P(GpuNormalization), P(GpuPod5Reads), P(GpuSampleRanges)
    tp, wp, ep, sp, xp, mp = P(GpuTrim), P(GpuWindows), P(GpuEvents), P(GpuSegmentation), P(GpuSpans), P(GpuMatch)
    t = {
        "vbz_is_error": (ctypes.c_bool, [u32]),
        "vbz_error_string": (ctypes.c_char_p, [u32]),
        "vbz_max_compressed_size": (u32, [u32, op]),
        "vbz_compress": (u32, [vp, u32, vp, u32, op]),
        "vbz_decompressed_size": (u32, [vp, u32, op]),
        "vbz_gpu_create": (vp, [c_int, vp]),
        "vbz_gpu_destroy": (None, [vp]),
        "vbz_gpu_stream": (vp, [vp]),
        "vbz_gpu_last_error": (ctypes.c_char_p, [vp]),
        "vbz_gpu_set_trailers": (None, [vp, c_int]),
        "vbz_gpu_synchronize": (c_int, [vp]),
        "vbz_gpu_compress_batch": (c_int, [vp, bp, op, c_int]),
        "vbz_gpu_decompress_signal_batch": (c_int, [vp, bp, op, c_int, fp]),
        "vbz_gpu_chunk_layout_batch": (c_int, [vp, u32, vp, cp, vp, vp, u64]),
        "vbz_gpu_decompress_chunks_batch": (c_int, [vp, bp, op, c_int, fp, cp, vp, vp, u64]),
        "vbz_gpu_signal_norm_batch": (c_int, [vp, bp, op, c_int, u32, np_, vp]),
        "vbz_gpu_decompress_signal_norm_batch": (c_int, [vp, bp, op, c_int, fp, np_, vp]),
        "vbz_gpu_decompress_chunks_norm_batch": (c_int, [vp, bp, op, c_int, fp, cp, vp, vp, u64, np_, vp]),
        "vbz_gpu_pod5_max_compressed_size": (u64, [u32]),
        "vbz_gpu_pod5_read_samples_batch": (c_int, [vp, u32, vp, rp, vp]),
        "vbz_gpu_pod5_decompress_chunks_batch": (c_int, [vp, bp, op, fp, cp, rp, vp, vp, u64, np_, vp]),
        "vbz_gpu_pod5_signal_norm_batch": (c_int, [vp, bp, op, u32, rp, np_, vp]),
        "vbz_gpu_pod5_decompress_signal_norm_batch": (c_int, [vp, bp, op, fp, rp, np_, vp]),
        "vbz_gpu_range_samples_batch": (c_int, [vp, u32, vp, gp, vp]),
        "vbz_gpu_decompress_chunks_range_batch": (c_int, [vp, bp, op, c_int, fp, cp, vp, vp, u64, np_, vp, gp]),
        "vbz_gpu_signal_norm_range_batch": (c_int, [vp, bp, op, c_int, u32, np_, vp, gp]),
        "vbz_gpu_pod5_decompress_chunks_range_batch": (c_int, [vp, bp, op, fp, cp, rp, vp, vp, u64, np_, vp, gp]),
        "vbz_gpu_pod5_signal_norm_range_batch": (c_int, [vp, bp, op, u32, rp, np_, vp, gp]),
        "vbz_gpu_signal_trim_batch": (c_int, [vp, bp, op, c_int, u32, np_, gp, tp, vp, vp]),
        "vbz_gpu_pod5_signal_trim_batch": (c_int, [vp, bp, op, u32, rp, np_, gp, tp, vp, vp]),
        "vbz_gpu_decompress_windows_batch": (c_int, [vp, bp, op, c_int, fp, wp, vp, np_, vp, gp]),
        "vbz_gpu_pod5_decompress_windows_batch": (c_int, [vp, bp, op, fp, rp, wp, vp, np_, vp, gp]),
        "vbz_gpu_signal_events_batch": (c_int, [vp, bp, op, c_int, fp, ep, vp, vp, np_, vp, gp]),
        "vbz_gpu_pod5_signal_events_batch": (c_int, [vp, bp, op, fp, rp, ep, vp, vp, np_, vp, gp]),
        "vbz_gpu_signal_segment_batch": (c_int, [vp, bp, op, c_int, u32, gp, sp, vp, vp]),
        "vbz_gpu_pod5_signal_segment_batch": (c_int, [vp, bp, op, u32, rp, gp, sp, vp, vp]),
        "vbz_gpu_signal_spans_batch": (c_int, [vp, bp, op, c_int, u32, np_, vp, gp, xp, vp, vp]),
        "vbz_gpu_pod5_signal_spans_batch": (c_int, [vp, bp, op, u32, rp, np_, vp, gp, xp, vp, vp]),
        "vbz_gpu_match_batch": (c_int, [vp, u32, vp, vp, mp, vp]),
        "vbz_gpu_signal_match_batch": (c_int, [vp, bp, op, c_int, fp, np_, vp, gp, mp, vp, vp]),
        "vbz_gpu_pod5_signal_match_batch": (c_int, [vp, bp, op, fp, rp, np_, vp, gp, mp, vp, vp]),
        "vbz_gpu_match_best_batch": (c_int, [vp, u32, vp, u32, u32, vp]),
        "vbz_gpu_match_path_batch": (c_int, [vp, u32, u32, vp, vp, mp, vp, P(GpuMatchPath), vp, vp]),
        "vbz_gpu_set_match_path_cap": (None, [vp, u64]),
        "vbz_gpu_query_valid_batch": (c_int, [vp, u32, vp, gp, u32, vp]),
        "vbz_gpu_events_query_batch": (c_int, [vp, u32, vp, ep, vp, P(GpuEventsQuery), vp, vp, vp]),
        "vbz_gpu_locate_levels_batch": (c_int, [vp, u32, u32, u32, u32, vp, vp, vp, vp, ep, vp, vp, vp, vp]),
        "vbz_gpu_squiggle_batch": (c_int, [vp, P(GpuSquiggle), vp, vp, vp, vp]),
        "vbz_gpu_levels_fit_batch": (c_int, [vp, u32, u32, P(GpuLocate), vp, vp, vp, vp, P(GpuLevelsFit), vp, vp, vp, vp, vp]),
        "vbz_gpu_svb_compress_batch": (c_int, [vp, bp, c_int, c_int, c_int]),
        "vbz_gpu_zstd_compress_batch": (c_int, [vp, bp, vp]),
        "vbz_gpu_zstd_decompress_batch": (c_int, [vp, bp]),
        "vbz_gpu_xxh64_batch": (c_int, [vp, bp, vp]),
        "vbz_gpu_pack_batch": (c_int, [vp, bp, u32, vp, u64, vp, vp]),
        "vbz_gpu_decompressed_size_batch": (c_int, [vp, bp, op, u32, vp, vp]),
        "vbz_gpu_synth_lengths": (c_int, [vp, u64, u64, u32, vp]),
        "vbz_gpu_synth_signal": (c_int, [vp, u64, u64, u32, vp, vp, vp]),
        "vbz_gpu_profile_enable": (None, [vp, c_int]),
        "vbz_gpu_profile_reset": (None, [vp]),
        "vbz_gpu_profile_read": (c_int, [vp, P(ctypes.c_char_p), P(u32), P(ctypes.c_double), c_int]),
        "vbz_gpu_decode_paths": (c_int, [vp, P(u32), P(u32)]),
        "vbz_gpu_decode_literals_ahead": (c_int, [vp]),
        "vbz_gpu_decode_span_paths": (c_int, [vp, P(u32)]),
        "vbz_gpu_version": (ctypes.c_char_p, []),
    }
    # the groups that share one signature
    for base, same in (("vbz_compress", ("vbz_decompress", "vbz_compress_sized", "vbz_decompress_sized")),
                       ("vbz_gpu_set_trailers", ("vbz_gpu_set_canonical", "vbz_gpu_set_checksum")),
                       ("vbz_gpu_compress_batch", ("vbz_gpu_decompress_batch",)),
                       ("vbz_gpu_svb_compress_batch", ("vbz_gpu_svb_decompress_batch",)),
                       ("vbz_gpu_synth_signal", ("vbz_gpu_synth_u32",))):
        for name in same:
            t[name] = t[base]
    # the locate forms: a vbz_gpu_locate in vbz_gpu_match's place, the arguments those of the match calls
    for name in ("vbz_gpu_match_batch", "vbz_gpu_signal_match_batch", "vbz_gpu_pod5_signal_match_batch", "vbz_gpu_match_path_batch"):
        t[name.replace("_match", "_locate", 1)] = (c_int, [P(GpuLocate) if a is mp else a for a in t[name][1]])
    # the _span twins: the hits are vbz_gpu_match_span, the arguments those of the cost-only calls
    for name in ("vbz_gpu_match_batch", "vbz_gpu_signal_match_batch", "vbz_gpu_pod5_signal_match_batch",
                 "vbz_gpu_locate_batch", "vbz_gpu_signal_locate_batch", "vbz_gpu_pod5_signal_locate_batch"):
        t[name.replace("_batch", "_span_batch")] = t[name]
    return t


PROTOTYPES = _prototypes()


def _pile_prototypes():
    """name -> (restype, argtypes) of every entry of PILE_API, as include/vbz_gpu_pile.h declares them: PROTOTYPES' shape."""
    c_int, vp, u32, P = ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER
    return {
        "vbz_gpu_levels_pile_batch": (c_int, [vp, u32, u32, P(GpuLocate), vp, vp, vp, vp, P(GpuLevelsPile), vp, vp]),
        "vbz_gpu_squiggle_kmers_batch": (c_int, [vp, P(GpuSquiggle), vp, vp]),
        "vbz_gpu_pile_kmers_batch": (c_int, [vp, P(GpuPileKmers), vp, vp, vp, vp]),
        "vbz_gpu_model_update_batch": (c_int, [vp, P(GpuModelUpdate), vp, vp, vp, vp]),
    }


PILE_PROTOTYPES = _pile_prototypes()
_lib = None


def load():
    """Load libvbz_hip.so and declare the prototypes. Raises RuntimeError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "%s is missing: build it with `python -m vbz_compression_amd.build` "
            "(there is no CPU fallback for the VBZ codec in this package)" % LIB_PATH
        )
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in list(PROTOTYPES.items()) + list(PILE_PROTOTYPES.items()):
        # (a name the library lacks is skipped: tools/ab_libs.py and tools/compare_libs.py load earlier builds through VBZ_HIP_LIB, and a
        # call of such a name fails at its first use)
        if hasattr(L, name):
            f = getattr(L, name)
            f.restype = restype
            f.argtypes = list(argtypes)
    _lib = L
    return L


def is_error(v):
    return int(v) >= VBZ_DEVICE_ERROR


def error_string(v):
    return load().vbz_error_string(int(v)).decode()
