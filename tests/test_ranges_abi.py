"""CPU tests of the sample-range entry points (include/vbz_gpu.h: vbz_gpu_sample_ranges): exported, declared with their struct and macros,
listed in _lib.GPU_API, and refused without a context before anything touches a device."""
import ctypes
import os
import re

from vbz_compression_amd import _lib, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vbz_gpu_range_samples_batch", "vbz_gpu_decompress_chunks_range_batch", "vbz_gpu_signal_norm_range_batch",
         "vbz_gpu_pod5_decompress_chunks_range_batch", "vbz_gpu_pod5_signal_norm_range_batch")


def header():
    return open(os.path.join(ROOT, "include", "vbz_gpu.h")).read()


def test_exported_declared_and_listed():
    L = _lib.load()
    text = header()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in _lib.GPU_API, name
        assert re.search(r"VBZ_EXPORT\s+int\s+" + name + r"\s*\(", text), name
        assert getattr(L, name).restype == ctypes.c_int and getattr(L, name).argtypes, name


def test_struct_layout():
    text = header()
    S = _lib.GpuSampleRanges
    assert ctypes.sizeof(S) == 24
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("begin", 0), ("end", 8), ("stats", 16), ("reserved", 20)]
    fields = re.search(r"typedef struct vbz_gpu_sample_ranges\s*\{(.*?)\}\s*vbz_gpu_sample_ranges;", text, re.S).group(1)
    names = re.findall(r"^\s*(?:const\s+)?uint32_t\*?\s+(\w+);", fields, re.M)
    assert names == [f[0] for f in S._fields_]


def test_macros():
    text = header()
    for name in ("VBZ_GPU_RANGE_STATS_RANGE", "VBZ_GPU_RANGE_STATS_READ"):
        m = re.search(r"#define\s+" + name + r"\s+(\w+)", text)
        assert m and int(m.group(1), 0) == getattr(_lib, name), name
    assert (_lib.VBZ_GPU_RANGE_STATS_RANGE, _lib.VBZ_GPU_RANGE_STATS_READ) == (0, 1)


def test_codec_methods_take_ranges():
    import inspect

    assert callable(batch.GpuCodec.range_samples)
    for name in ("decompress_chunks", "decompress_packed_chunks", "signal_norm", "pod5_decompress_chunks", "pod5_signal_norm"):
        p = inspect.signature(getattr(batch.GpuCodec, name)).parameters
        assert {"begin", "end", "stats"} <= set(p), name


def test_null_context_or_batch_is_minus_one():
    L = _lib.load()
    b = _lib.GpuBatch()
    opts = _lib.CompressionOptions(True, 2, 1, 1)
    popts = batch.pod5_options()
    f = _lib.GpuSignalFormat()
    f.out_type = _lib.VBZ_GPU_SIGNAL_F16
    f.is_signed = 1
    ch = _lib.GpuChunking()
    ch.chunk_len, ch.step, ch.mode = 16, 8, _lib.VBZ_GPU_CHUNK_PAD
    m = batch.MED_MAD.c_struct()
    r = _lib.GpuPod5Reads()
    g = _lib.GpuSampleRanges()
    assert L.vbz_gpu_range_samples_batch(None, 0, None, ctypes.byref(g), None) == -1
    for ctx_b in ((None, ctypes.byref(b)), (None, None)):
        assert L.vbz_gpu_decompress_chunks_range_batch(*ctx_b, ctypes.byref(opts), 0, ctypes.byref(f), ctypes.byref(ch), None, None, 0, ctypes.byref(m), None,
                                                       ctypes.byref(g)) == -1
        assert L.vbz_gpu_signal_norm_range_batch(*ctx_b, ctypes.byref(opts), 0, 1, ctypes.byref(m), None, ctypes.byref(g)) == -1
        assert L.vbz_gpu_pod5_decompress_chunks_range_batch(*ctx_b, ctypes.byref(popts), ctypes.byref(f), ctypes.byref(ch), ctypes.byref(r), None, None, 0,
                                                            ctypes.byref(m), None, ctypes.byref(g)) == -1
        assert L.vbz_gpu_pod5_signal_norm_range_batch(*ctx_b, ctypes.byref(popts), 1, ctypes.byref(r), ctypes.byref(m), None, ctypes.byref(g)) == -1
