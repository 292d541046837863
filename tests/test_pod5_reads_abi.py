"""CPU tests of the entry points over POD5 reads of several rows (include/vbz_gpu.h: vbz_gpu_pod5_reads): exported, declared with their
struct, and refused without a context before anything touches a device."""
import ctypes
import os
import re

from vbz_compression_amd import _lib, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vbz_gpu_pod5_read_samples_batch", "vbz_gpu_pod5_decompress_chunks_batch", "vbz_gpu_pod5_signal_norm_batch",
         "vbz_gpu_pod5_decompress_signal_norm_batch")


def header():
    return open(os.path.join(ROOT, "include", "vbz_gpu.h")).read()


def test_exported_and_declared():
    L = _lib.load()
    text = header()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in _lib.GPU_API, name
        assert re.search(r"VBZ_EXPORT\s+int\s+" + name + r"\s*\(", text), name
        assert getattr(L, name).restype == ctypes.c_int and getattr(L, name).argtypes, name


def test_struct_layout():
    text = header()
    S = _lib.GpuPod5Reads
    assert ctypes.sizeof(S) == 24
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("n_reads", 0), ("reserved", 4), ("first_row", 8), ("read_result", 16)]
    fields = re.search(r"typedef struct vbz_gpu_pod5_reads\s*\{(.*?)\}\s*vbz_gpu_pod5_reads;", text, re.S).group(1)
    names = re.findall(r"^\s*(?:const\s+)?uint32_t\*?\s+(\w+);", fields, re.M)
    assert names == [f[0] for f in S._fields_]


def test_codec_methods():
    for name in ("pod5_decompress_chunks", "pod5_signal_norm", "pod5_decompress_signal_norm"):
        assert callable(getattr(batch.GpuCodec, name)), name


def test_null_context_or_batch_is_minus_one():
    L = _lib.load()
    b = _lib.GpuBatch()
    opts = batch.pod5_options()
    f = _lib.GpuSignalFormat()
    f.out_type = _lib.VBZ_GPU_SIGNAL_F16
    f.is_signed = 1
    ch = _lib.GpuChunking()
    ch.chunk_len, ch.step, ch.mode = 16, 8, _lib.VBZ_GPU_CHUNK_PAD
    m = batch.MED_MAD.c_struct()
    r = _lib.GpuPod5Reads()
    assert L.vbz_gpu_pod5_read_samples_batch(None, 0, None, ctypes.byref(r), None) == -1
    for ctx_b in ((None, ctypes.byref(b)), (None, None)):
        assert L.vbz_gpu_pod5_decompress_chunks_batch(*ctx_b, ctypes.byref(opts), ctypes.byref(f), ctypes.byref(ch), ctypes.byref(r), None, None, 0,
                                                      ctypes.byref(m), None) == -1
        assert L.vbz_gpu_pod5_signal_norm_batch(*ctx_b, ctypes.byref(opts), 1, ctypes.byref(r), ctypes.byref(m), None) == -1
        assert L.vbz_gpu_pod5_decompress_signal_norm_batch(*ctx_b, ctypes.byref(opts), ctypes.byref(f), ctypes.byref(r), ctypes.byref(m), None) == -1
