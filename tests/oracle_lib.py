"""ctypes binding of the CPU ORACLE (oracle/liboracle.so).  Test infrastructure only:
imported by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg, never by the product."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
ERRORS = {
    0xFFFFFFFF: "VBZ_ZSTD_ERROR",
    0xFFFFFFFE: "VBZ_INPUT_SIZE_ERROR",
    0xFFFFFFFD: "VBZ_INTEGER_SIZE_ERROR",
    0xFFFFFFFC: "VBZ_DESTINATION_SIZE_ERROR",
    0xFFFFFFFB: "VBZ_STREAMVBYTE_STREAM_ERROR",
    0xFFFFFFFA: "VBZ_VERSION_ERROR",
    0xFFFFFFF9: "VBZ_OUT_OF_MEMORY_ERROR",
}
FIRST_ERROR = 0xFFFFFFF9


class Options(ctypes.Structure):
    _fields_ = [
        ("perform_delta_zig_zag", ctypes.c_bool),
        ("integer_size", ctypes.c_uint),
        ("zstd_compression_level", ctypes.c_uint),
        ("vbz_version", ctypes.c_uint),
    ]


def build_oracle():
    so = os.path.join(ORACLE_DIR, "liboracle.so")
    srcs = [os.path.join(ORACLE_DIR, f) for f in ("vbz_oracle.c", "zstd_restate.c", "vbz_oracle_bench.c", "vbz_oracle_fuzz.c", "vbz_oracle_simd.c", "vbz_oracle.h", "Makefile")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["make", "-C", ORACLE_DIR, "-s"])
    return so


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build_oracle())
        vp, u32, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t
        op = ctypes.POINTER(Options)
        L.vbo_max_streamvbyte_size.restype = u32
        L.vbo_max_streamvbyte_size.argtypes = [sz, u32]
        for name in ("vbo_streamvbyte_compress", "vbo_streamvbyte_decompress"):
            f = getattr(L, name)
            f.restype = u32
            f.argtypes = [vp, u32, vp, u32, ctypes.c_int, ctypes.c_bool, ctypes.c_uint]
        L.vbo_max_compressed_size.restype = u32
        L.vbo_max_compressed_size.argtypes = [u32, op]
        for name in ("vbo_compress", "vbo_decompress", "vbo_compress_sized", "vbo_decompress_sized"):
            f = getattr(L, name)
            f.restype = u32
            f.argtypes = [vp, u32, vp, u32, op]
        L.vbo_decompressed_size.restype = u32
        L.vbo_decompressed_size.argtypes = [vp, u32, op]
        L.vbo_error_string.restype = ctypes.c_char_p
        L.vbo_error_string.argtypes = [u32]
        L.vbo_is_error.restype = ctypes.c_bool
        L.vbo_is_error.argtypes = [u32]
        L.vbo_filter.restype = sz
        L.vbo_filter.argtypes = [ctypes.c_uint, sz, ctypes.POINTER(ctypes.c_uint), sz, ctypes.POINTER(sz), ctypes.POINTER(vp)]
        L.vbo_zstd_version.restype = ctypes.c_char_p
        L.vbo_zstd_compress.restype = sz
        L.vbo_zstd_compress.argtypes = [vp, sz, vp, sz, ctypes.c_int]
        L.vbo_zstd_decompress.restype = sz
        L.vbo_zstd_decompress.argtypes = [vp, sz, vp, sz]
        L.vbo_zstd_bound.restype = sz
        L.vbo_zstd_bound.argtypes = [sz]
        L.vbo_zstd_content_size.restype = ctypes.c_ulonglong
        L.vbo_zstd_content_size.argtypes = [vp, sz]
        L.vbo_zstd_restate_decompress.restype = sz
        L.vbo_zstd_restate_decompress.argtypes = [vp, sz, vp, sz]
        L.vbo_zstd_restate_census.restype = sz
        L.vbo_zstd_restate_census.argtypes = [vp, sz, vp, sz]
        L.vbo_zstd_restate_sequences.restype = sz
        L.vbo_zstd_restate_sequences.argtypes = [vp, sz, vp, sz, ctypes.POINTER(sz), vp, sz]
        L.vbo_zstd_census_count.restype = ctypes.c_int
        L.vbo_zstd_census_name.restype = ctypes.c_char_p
        L.vbo_zstd_census_name.argtypes = [ctypes.c_int]
        L.vbo_zstd_census_is_max.restype = ctypes.c_int
        L.vbo_zstd_census_is_max.argtypes = [ctypes.c_int]
        L.vbo_mix64.restype = ctypes.c_uint64
        L.vbo_mix64.argtypes = [ctypes.c_uint64]
        L.vbo_synth_read_length.restype = u32
        L.vbo_synth_read_length.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
        L.vbo_synth_signal.restype = None
        L.vbo_synth_signal.argtypes = [ctypes.c_uint64, ctypes.c_uint64, vp, sz]
        L.vbo_synth_u32.restype = None
        L.vbo_synth_u32.argtypes = [ctypes.c_uint64, ctypes.c_uint64, vp, sz]
        L.vbo_bench_roundtrip.restype = ctypes.c_int
        L.vbo_bench_roundtrip.argtypes = [u32, ctypes.c_int, ctypes.c_double, op, ctypes.POINTER(ctypes.c_double)]
        L.vbo_bench_roundtrip_u32.restype = ctypes.c_int
        L.vbo_bench_roundtrip_u32.argtypes = [u32, u32, ctypes.c_int, ctypes.c_double, op, ctypes.POINTER(ctypes.c_double)]
        L.vbo_simd_available.restype = ctypes.c_int
        L.vbo_use_simd_svb.restype = None
        L.vbo_use_simd_svb.argtypes = [ctypes.c_int]
        for name in ("vbo_i16zz_compress_simd",):
            getattr(L, name).restype = u32
            getattr(L, name).argtypes = [vp, u32, vp]
        L.vbo_i16zz_decompress_simd.restype = u32
        L.vbo_i16zz_decompress_simd.argtypes = [vp, u32, vp, u32]
        L.vbo_debug_fse_read_ncount.restype = ctypes.c_int
        L.vbo_debug_fse_read_ncount.argtypes = [vp, sz, vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        L.vbo_debug_fse_build.restype = ctypes.c_int
        L.vbo_debug_fse_build.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp]
        L.vbo_debug_huf_lengths.restype = ctypes.c_int
        L.vbo_debug_huf_lengths.argtypes = [vp, sz, vp, ctypes.POINTER(ctypes.c_int)]
        L.vbo_debug_lit_header.restype = ctypes.c_int
        L.vbo_debug_lit_header.argtypes = [vp, sz, vp]
        L.vbo_debug_nseq.restype = ctypes.c_int
        L.vbo_debug_nseq.argtypes = [vp, sz, vp]
        L.vbo_fuzz_max_destination.restype = u32
        L.vbo_fuzz_max_destination.argtypes = [u32, op]
        L.vbo_fuzz_decompress_sweep.restype = ctypes.c_int
        L.vbo_fuzz_decompress_sweep.argtypes = [vp, u32, op, u32, vp]
        _lib = L
    return _lib


def fuzz_sweep(data, opts):
    """Replay of the reference fuzz target's decompress half for one input and option set (oracle/vbz_oracle_fuzz.c):
    returns (max_destination, results[max_destination + 1, 2]) -- column 0 vbz_decompress, column 1 vbz_decompress_sized."""
    a, p, n = _buf(np.frombuffer(bytes(data), np.uint8))
    G = lib().vbo_fuzz_max_destination(n, ctypes.byref(opts))
    res = np.zeros((G + 1, 2), np.uint32)
    rc = lib().vbo_fuzz_decompress_sweep(p, n, ctypes.byref(opts), G, res.ctypes.data)
    assert rc == 0
    return G, res


def options(zigzag=True, size=2, level=1, version=0):
    return Options(bool(zigzag), int(size), int(level), int(version))


def _buf(a):
    a = np.ascontiguousarray(a)
    return a, (a.ctypes.data if a.size else None), a.nbytes


def is_error(v):
    return v >= FIRST_ERROR


def svb_compress(arr, size, zigzag, version=0):
    a, p, n = _buf(arr)
    cap = lib().vbo_max_streamvbyte_size(size, n)
    assert not is_error(cap), ERRORS.get(cap)
    out = np.zeros(cap + 32, np.uint8)
    r = lib().vbo_streamvbyte_compress(p, n, out.ctypes.data, cap, size, zigzag, version)
    if is_error(r):
        return r
    return out[:r].copy()


def svb_decompress(buf, nbytes, size, zigzag, version=0):
    a, p, n = _buf(np.frombuffer(bytes(buf), np.uint8) if not isinstance(buf, np.ndarray) else buf)
    out = np.zeros(max(nbytes, 1), np.uint8)
    r = lib().vbo_streamvbyte_decompress(p, n, out.ctypes.data, nbytes, size, zigzag, version)
    if is_error(r):
        return r
    return out[:r].copy()


SIMD_DECLINED = 0xFFFFFF9C   # (vbo_size_t)-100: not a stream the SSSE3 decoder takes


def simd_available():
    return bool(lib().vbo_simd_available())


def i16zz_compress_simd(arr):
    """The SSSE3 form of the int16 zig-zag stage (oracle/vbz_oracle_simd.c: CPU baseline leg only)."""
    a, p, n = _buf(arr)
    out = np.zeros(n // 2 // 4 + n + 64, np.uint8)
    r = lib().vbo_i16zz_compress_simd(p, n, out.ctypes.data)
    return out[:r].copy()


def i16zz_decompress_simd(buf, nbytes):
    a, p, n = _buf(np.frombuffer(bytes(buf), np.uint8) if not isinstance(buf, np.ndarray) else buf)
    src = np.zeros(n + 64, np.uint8)   # (the vector loads stay inside the stream by the 32-byte rule; slack for safety)
    src[:n] = a.view(np.uint8).reshape(-1)[:n]
    out = np.zeros(max(nbytes, 1) + 16, np.uint8)
    r = lib().vbo_i16zz_decompress_simd(src.ctypes.data, n, out.ctypes.data, nbytes)
    if r >= FIRST_ERROR or r == SIMD_DECLINED:
        return r
    return out[:r].copy()


def max_compressed_size(nbytes, opts):
    return lib().vbo_max_compressed_size(nbytes, ctypes.byref(opts))


def compress(arr, opts, sized=False):
    a, p, n = _buf(arr)
    cap = max_compressed_size(n, opts)
    if is_error(cap):
        return cap
    out = np.zeros(cap + 32, np.uint8)
    fn = lib().vbo_compress_sized if sized else lib().vbo_compress
    r = fn(p, n, out.ctypes.data, cap, ctypes.byref(opts))
    if is_error(r):
        return r
    return out[:r].copy()


def decompress(buf, nbytes, opts, sized=False):
    a, p, n = _buf(buf if isinstance(buf, np.ndarray) else np.frombuffer(bytes(buf), np.uint8))
    out = np.zeros(max(nbytes, 1), np.uint8)
    fn = lib().vbo_decompress_sized if sized else lib().vbo_decompress
    r = fn(p, n, out.ctypes.data, nbytes, ctypes.byref(opts))
    if is_error(r):
        return r
    return out[:r].copy()


def zstd_compress(data, level=1):
    a, p, n = _buf(data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), np.uint8))
    cap = lib().vbo_zstd_bound(n)
    out = np.zeros(cap + 8, np.uint8)
    r = lib().vbo_zstd_compress(out.ctypes.data, cap, p, n, level)
    assert r != 2**64 - 1
    return out[:r].copy()


def zstd_decompress(frame, cap):
    a, p, n = _buf(frame if isinstance(frame, np.ndarray) else np.frombuffer(bytes(frame), np.uint8))
    out = np.zeros(max(cap, 1), np.uint8)
    r = lib().vbo_zstd_decompress(out.ctypes.data, cap, p, n)
    if r == 2**64 - 1:
        return None
    return out[:r].copy()


def zstd_restate_decompress(frame, cap):
    a, p, n = _buf(frame if isinstance(frame, np.ndarray) else np.frombuffer(bytes(frame), np.uint8))
    out = np.zeros(max(cap, 1), np.uint8)
    r = lib().vbo_zstd_restate_decompress(out.ctypes.data, cap, p, n)
    if r == 2**64 - 1:
        return None
    return out[:r].copy()


def census_names():
    """The census counters' names, in the order of oracle/vbz_oracle.h's VBO_CENSUS."""
    return [lib().vbo_zstd_census_name(k).decode() for k in range(lib().vbo_zstd_census_count())]


def census_maxima():
    """The names of the counters that are maxima (merged over frames with max; every other one adds up)."""
    return {lib().vbo_zstd_census_name(k).decode() for k in range(lib().vbo_zstd_census_count()) if lib().vbo_zstd_census_is_max(k)}


def zstd_census(frame):
    """{counter name: value} of what the restated decoder meets in the buffer's frames (oracle/vbz_oracle.h, VBO_CENSUS), with the content
    size under "content_size"; None where the restated decoder refuses the buffer."""
    a, p, n = _buf(frame if isinstance(frame, np.ndarray) else np.frombuffer(bytes(frame), np.uint8))
    names = census_names()
    c = np.zeros(len(names), np.uint64)
    r = lib().vbo_zstd_restate_census(p, n, c.ctypes.data, len(names))
    if r == 2**64 - 1:
        return None
    out = {k: int(v) for k, v in zip(names, c)}
    out["content_size"] = int(r)
    return out


# oracle/vbz_oracle.h: VboSeqBlock, VboSeq
SEQ_BLOCK = np.dtype([("begin", "<u8"), ("end", "<u8"), ("ordinal", "<u4"), ("type", "<u4"), ("literals", "<u4"), ("nseq", "<u4")])
SEQ = np.dtype([("pos", "<u8"), ("unread", "<i8"), ("block", "<u4"), ("ll", "<u4"), ("ml", "<u4"), ("offset", "<u4"), ("ofv", "<u4"),
                ("ll_state", "<u2"), ("ml_state", "<u2"), ("ll_code", "u1"), ("of_code", "u1"), ("ml_code", "u1"), ("reserved0", "u1"),
                ("reserved1", "<u4")])
assert SEQ_BLOCK.itemsize == 32 and SEQ.itemsize == 48


def zstd_sequences(frame):
    """(blocks, seqs): every block and every sequence of the buffer's frames as the restated decoder meets them (oracle/vbz_oracle.h,
    vbo_zstd_restate_sequences), two structured arrays of SEQ_BLOCK and SEQ; None where the restated decoder refuses the buffer."""
    a, p, n = _buf(frame if isinstance(frame, np.ndarray) else np.frombuffer(bytes(frame), np.uint8))
    nb = ctypes.c_size_t(0)
    ns = lib().vbo_zstd_restate_sequences(p, n, None, 0, ctypes.byref(nb), None, 0)
    if ns == 2**64 - 1:
        return None
    blocks, seqs = np.zeros(nb.value, SEQ_BLOCK), np.zeros(ns, SEQ)
    r = lib().vbo_zstd_restate_sequences(p, n, blocks.ctypes.data if nb.value else None, nb.value, ctypes.byref(nb), seqs.ctypes.data if ns else None, ns)
    assert r == ns and nb.value == len(blocks)
    return blocks, seqs


def zstd_content_size(frame):
    a, p, n = _buf(frame if isinstance(frame, np.ndarray) else np.frombuffer(bytes(frame), np.uint8))
    return lib().vbo_zstd_content_size(p, n)


def synth_signal(seed, read_index, n):
    out = np.zeros(n, np.int16)
    lib().vbo_synth_signal(seed, read_index, out.ctypes.data, n)
    return out


def synth_u32(seed, read_index, n):
    out = np.zeros(n, np.uint32)
    lib().vbo_synth_u32(seed, read_index, out.ctypes.data, n)
    return out


def synth_read_length(seed, read_index):
    return lib().vbo_synth_read_length(seed, read_index)


def fnv1a64(data):
    h = 0xCBF29CE484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def bench_roundtrip(n_reads, threads, min_seconds, opts, u32_count=0, simd=False):
    """Threaded CPU timing of encode+decode over reads [0, n_reads) of the synthetic workload (u32_count: buffers of that
    many uint32 values of the config-4 generator instead of int16 reads).  simd: the int16 zig-zag stage in its SSSE3 form."""
    out = (ctypes.c_double * 6)()
    lib().vbo_use_simd_svb(1 if simd else 0)
    try:
        if u32_count:
            rc = lib().vbo_bench_roundtrip_u32(n_reads, u32_count, threads, min_seconds, ctypes.byref(opts), out)
        else:
            rc = lib().vbo_bench_roundtrip(n_reads, threads, min_seconds, ctypes.byref(opts), out)
    finally:
        lib().vbo_use_simd_svb(0)
    if rc != 0:
        raise RuntimeError("oracle bench failed (%d)" % rc)
    return dict(raw_bytes=out[0], comp_bytes=out[1], best_s=out[2], enc_thread_s=out[3], dec_thread_s=out[4], passes=int(out[5]))


# ---- libzstd itself for chosen block layouts (ctypes on libzstd.so.1: the pinned dependency, no header needed) --------------------------
# A one-shot ZSTD_compress cuts its input into blocks of block_max = min(window, 128 KiB) bytes; a writer that flushes
# (ZSTD_compressStream2 with ZSTD_e_flush, as streaming writers and libzstd >= 1.5 do) ends a block wherever it flushes.
BLOCK_MAX = 128 << 10
# ZSTD_cParameter (zstd.h of 1.4.8; the numbers are part of the library's ABI)
ZSTD_c_compressionLevel, ZSTD_c_windowLog, ZSTD_c_hashLog, ZSTD_c_chainLog, ZSTD_c_searchLog = 100, 101, 102, 103, 104
ZSTD_c_minMatch, ZSTD_c_targetLength, ZSTD_c_strategy, ZSTD_c_enableLongDistanceMatching = 105, 106, 107, 160
ZSTD_c_contentSizeFlag, ZSTD_c_checksumFlag = 200, 201
ZSTD_e_continue = 0
ZSTD_e_flush, ZSTD_e_end = 1, 2


class _ZBuf(ctypes.Structure):   # ZSTD_inBuffer / ZSTD_outBuffer
    _fields_ = [("ptr", ctypes.c_void_p), ("size", ctypes.c_size_t), ("pos", ctypes.c_size_t)]


_zstd = None


def libzstd():
    global _zstd
    if _zstd is None:
        L = ctypes.CDLL("libzstd.so.1")
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        L.ZSTD_isError.restype = ctypes.c_uint
        L.ZSTD_isError.argtypes = [sz]
        L.ZSTD_compressBound.restype = sz
        L.ZSTD_compressBound.argtypes = [sz]
        L.ZSTD_createCCtx.restype = vp
        L.ZSTD_freeCCtx.argtypes = [vp]
        L.ZSTD_CCtx_setParameter.restype = sz
        L.ZSTD_CCtx_setParameter.argtypes = [vp, ctypes.c_int, ctypes.c_int]
        L.ZSTD_CCtx_setPledgedSrcSize.restype = sz
        L.ZSTD_CCtx_setPledgedSrcSize.argtypes = [vp, ctypes.c_ulonglong]
        L.ZSTD_compressStream2.restype = sz
        L.ZSTD_compressStream2.argtypes = [vp, ctypes.POINTER(_ZBuf), ctypes.POINTER(_ZBuf), ctypes.c_int]
        L.ZSTD_compress2.restype = sz
        L.ZSTD_compress2.argtypes = [vp, vp, sz, vp, sz]
        L.ZSTD_createDCtx.restype = vp
        L.ZSTD_freeDCtx.argtypes = [vp]
        L.ZSTD_decompressBegin.restype = sz
        L.ZSTD_decompressBegin.argtypes = [vp]
        L.ZSTD_nextSrcSizeToDecompress.restype = sz
        L.ZSTD_nextSrcSizeToDecompress.argtypes = [vp]
        L.ZSTD_nextInputType.restype = ctypes.c_int
        L.ZSTD_nextInputType.argtypes = [vp]
        L.ZSTD_decompressContinue.restype = sz
        L.ZSTD_decompressContinue.argtypes = [vp, vp, sz, vp, sz]
        _zstd = L
    return _zstd


def zstd_compress_params(data, params, cuts=(), pledge=True):
    """A libzstd frame of `data` under `params` ({ZSTD_cParameter number: value}, set in the dict's order), its blocks ending at every cut
    (a flush) -- and wherever libzstd itself ends one.  cuts: strictly increasing, each in (0, len(data)]; a cut at len(data) flushes
    everything before the frame is ended, which leaves an empty last block.  pledge: the source size is declared in advance (a content
    size in the header unless ZSTD_c_contentSizeFlag is 0); without it the frame is streamed and has none.  Pledged and without cuts:
    ZSTD_compress2."""
    a = np.ascontiguousarray(data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), np.uint8)).view(np.uint8).reshape(-1)
    n = a.nbytes
    cuts = [int(c) for c in cuts]
    if any(not 0 < c <= n for c in cuts) or any(x >= y for x, y in zip(cuts, cuts[1:])):
        raise ValueError("cuts must increase strictly inside (0, %d]: %s" % (n, cuts))
    Z = libzstd()
    cap = Z.ZSTD_compressBound(n) + 64 * (len(cuts) + 1) + 64
    out = np.zeros(cap, np.uint8)
    cc = Z.ZSTD_createCCtx()
    assert cc
    try:
        for p, v in params.items():
            assert not Z.ZSTD_isError(Z.ZSTD_CCtx_setParameter(cc, int(p), int(v))), (p, v)
        if pledge:
            assert not Z.ZSTD_isError(Z.ZSTD_CCtx_setPledgedSrcSize(cc, n))
        keep = a if n else np.zeros(1, np.uint8)   # (a valid pointer for the empty content too)
        src = keep.ctypes.data
        if not cuts and pledge:
            r = Z.ZSTD_compress2(cc, out.ctypes.data, cap, src if n else None, n)
            assert not Z.ZSTD_isError(r), r
            return out[:r].copy()
        ob = _ZBuf(out.ctypes.data, cap, 0)
        # (a frame ended by the first call would get that call's input as its pledge: an unpledged frame's content goes in ahead of the end)
        steps = [(c, ZSTD_e_flush) for c in cuts] + ([(n, ZSTD_e_continue)] if not pledge and not cuts else []) + [(n, ZSTD_e_end)]
        prev = 0
        for c, mode in steps:
            ib = _ZBuf(src + prev, c - prev, 0)
            while True:
                r = Z.ZSTD_compressStream2(cc, ctypes.byref(ob), ctypes.byref(ib), mode)
                assert not Z.ZSTD_isError(r), r
                if ib.pos == ib.size and (r == 0 or mode == ZSTD_e_continue):
                    break
                assert ob.pos < cap
            prev = c
        return out[: ob.pos].copy()
    finally:
        Z.ZSTD_freeCCtx(cc)


def zstd_compress_cuts(data, cuts=(), level=1, window_log=0, checksum=False):
    """A libzstd frame of `data` (content size in the header) whose blocks end at every cut -- and wherever libzstd itself ends one:
    every block_max bytes of a stretch between cuts.  cuts: strictly increasing, each in (0, len(data)).  No cuts: ZSTD_compress2."""
    n = (data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), np.uint8)).nbytes
    cuts = [int(c) for c in cuts]
    if any(not 0 < c < n for c in cuts) or any(x >= y for x, y in zip(cuts, cuts[1:])):
        raise ValueError("cuts must increase strictly inside (0, %d): %s" % (n, cuts))
    return zstd_compress_params(data, {ZSTD_c_compressionLevel: level, ZSTD_c_windowLog: window_log, ZSTD_c_checksumFlag: 1 if checksum else 0}, cuts)


def zstd_block_ends(frame, cap):
    """Where every block of a one-frame buffer ends in the content, by libzstd's bufferless decoder (None: libzstd refuses the frame)."""
    f = np.ascontiguousarray(frame if isinstance(frame, np.ndarray) else np.frombuffer(bytes(frame), np.uint8))
    Z = libzstd()
    out = np.zeros(max(int(cap), 1), np.uint8)
    dc = Z.ZSTD_createDCtx()
    assert dc
    ends, ipos, opos = [], 0, 0
    try:
        if Z.ZSTD_isError(Z.ZSTD_decompressBegin(dc)):
            return None
        while True:
            need = Z.ZSTD_nextSrcSizeToDecompress(dc)
            if need == 0:
                return ends
            if ipos + need > len(f):
                return None
            kind = Z.ZSTD_nextInputType(dc)   # ZSTDnit_block = 2, ZSTDnit_lastBlock = 3
            r = Z.ZSTD_decompressContinue(dc, out.ctypes.data + opos, len(out) - opos, f.ctypes.data + ipos, need)
            if Z.ZSTD_isError(r):
                return None
            ipos += need
            opos += r
            if kind in (2, 3):
                ends.append(opos)
    finally:
        Z.ZSTD_freeDCtx(dc)


def zstd_frame_geometry(frame):
    """(header bytes, content size, block_max, checksum flag) of a frame with a content size -- RFC 8878 3.1.1.1, as the device reads it."""
    f = bytes(frame[:18])
    fhd = f[4]
    single, fcs_flag = (fhd >> 5) & 1, fhd >> 6
    pos = 5
    window = 0
    if not single:
        wd = f[pos]
        pos += 1
        wlog = 10 + (wd >> 3)
        window = (1 << wlog) + ((1 << wlog) >> 3) * (wd & 7)
    pos += (0, 1, 2, 4)[fhd & 3]
    fsz = (1 if single else 0, 2, 4, 8)[fcs_flag]
    assert fsz, "no content size"
    fcs = int.from_bytes(f[pos : pos + fsz], "little") + (256 if fsz == 2 else 0)
    pos += fsz
    if single:
        window = fcs
    return pos, fcs, min(window, BLOCK_MAX), (fhd >> 2) & 1


def ref_literal_units(frame, max_units=4):
    """A restatement, in outline, of which blocks of a reference-written frame get their literals decoded beside the chain walk (a
    "unit": compressed literals in four streams of at least 4 x 384 bytes, under a tree of their own or an earlier unit's; at most four a
    frame) and of where those literals are put ahead of the decoder if the block is not the frame's last: at a guessed block end
    G = min((ordinal + 1) x block_max, content size), the frame's content size for its last block.  One dict per unit: ordinal, last,
    regen (the literals' count), guess G and the range [G - regen, G) they would be written to.  Not a model of the device's output: it
    is here to show that a frame holds units whose ranges overlap."""
    f = bytes(frame)
    pos, fcs, bmax, _ = zstd_frame_geometry(f)
    units = []
    have_tree = False
    bidx = 0
    while len(units) < max_units and pos + 3 <= len(f):
        bh = int.from_bytes(f[pos : pos + 3], "little")
        last, btype, bsize = bh & 1, (bh >> 1) & 3, bh >> 3
        if btype == 3:
            break
        blk = pos + 3
        unit = False
        if btype == 2 and 5 <= bsize < BLOCK_MAX:
            v = int.from_bytes(f[blk : blk + 5], "little")
            ltype, fmt = v & 3, (v >> 2) & 3
            if ltype >= 2 and fmt != 0:
                lh, rb, cb = {1: (3, 10, 10), 2: (4, 14, 14), 3: (5, 18, 18)}[fmt]
                regen, csize = (v >> 4) & ((1 << rb) - 1), (v >> (4 + rb)) & ((1 << cb) - 1)
                tree = 0
                if ltype == 2:
                    hb = f[blk + lh]
                    tree = 1 + ((hb - 127) + 1) // 2 if hb >= 128 else 1 + hb
                ok = regen and csize > tree + 10 and (ltype == 2 or have_tree)
                if ok:
                    q = blk + lh + tree
                    s1, s2, s3 = (int.from_bytes(f[q + 2 * k : q + 2 * k + 2], "little") for k in range(3))
                    s4 = csize - tree - 6 - s1 - s2 - s3
                    if min(s1, s2, s3, s4) >= 4 * 384:
                        g = fcs if last else min((bidx + 1) * bmax, fcs)
                        units.append(dict(ordinal=bidx, last=bool(last), regen=regen, guess=g, range=(g - regen, g) if g >= regen else None))
                        unit = True
                        if ltype == 2:
                            have_tree = True
            if not unit and ltype == 2:
                have_tree = False
        pos = blk + (1 if btype == 1 else bsize)
        bidx += 1
        if last:
            break
    return units


def overlapping_units(units):
    """Pairs (i, j) of units whose write ranges overlap: a wrong guess of one puts its literals inside the other's range."""
    pairs = []
    for i, a in enumerate(units):
        for j in range(i + 1, len(units)):
            b = units[j]
            if a["range"] and b["range"] and a["range"][0] < b["range"][1] and b["range"][0] < a["range"][1]:
                pairs.append((i, j))
    return pairs
