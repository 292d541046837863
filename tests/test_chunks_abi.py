"""CPU tests of the model-input chunk entry points (include/vbz_gpu.h: vbz_gpu_chunk_layout_batch, vbz_gpu_decompress_chunks_batch):
exported, declared with their chunking struct and macros, and refused without a context before anything touches a device."""
import ctypes
import os
import re

from vbz_compression_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vbz_gpu_chunk_layout_batch", "vbz_gpu_decompress_chunks_batch")


def header():
    return open(os.path.join(ROOT, "include", "vbz_gpu.h")).read()


def test_exported_and_declared():
    L = _lib.load()
    text = header()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in _lib.GPU_API, name
        assert re.search(r"VBZ_EXPORT\s+int\s+" + name + r"\s*\(", text), name


def test_macros_and_struct():
    text = header()
    for macro, value in (("VBZ_GPU_CHUNK_PAD", 0), ("VBZ_GPU_CHUNK_END", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), text), macro
        assert getattr(_lib, macro) == value
    assert ctypes.sizeof(_lib.GpuChunking) == 24
    fields = re.search(r"typedef struct vbz_gpu_chunking\s*\{(.*?)\}\s*vbz_gpu_chunking;", text, re.S).group(1)
    names = re.findall(r"^\s*(?:uint32_t|float)\s+(\w+);", fields, re.M)
    assert names == [f[0] for f in _lib.GpuChunking._fields_]


def test_null_context_or_batch_is_minus_one():
    L = _lib.load()
    b = _lib.GpuBatch()
    opts = _lib.CompressionOptions(True, 2, 1, 1)
    f = _lib.GpuSignalFormat()
    f.out_type = _lib.VBZ_GPU_SIGNAL_F16
    f.is_signed = 1
    ch = _lib.GpuChunking()
    ch.chunk_len, ch.step, ch.mode = 16, 8, _lib.VBZ_GPU_CHUNK_PAD
    dec = L.vbz_gpu_decompress_chunks_batch
    assert dec(None, ctypes.byref(b), ctypes.byref(opts), 0, ctypes.byref(f), ctypes.byref(ch), None, None, 0) == -1
    assert dec(None, None, ctypes.byref(opts), 1, ctypes.byref(f), ctypes.byref(ch), None, None, 0) == -1
    assert dec(None, None, None, 0, None, None, None, None, 0) == -1
    assert L.vbz_gpu_chunk_layout_batch(None, 0, None, ctypes.byref(ch), None, None, 0) == -1
    assert L.vbz_gpu_chunk_layout_batch(None, 4, None, None, None, None, 0) == -1
