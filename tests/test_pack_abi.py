"""CPU tests of the dense-arena entry points (include/vbz_gpu.h: vbz_gpu_pack_batch, vbz_gpu_decompressed_size_batch): exported,
declared, and refused without a context before anything touches a device."""
import ctypes
import os
import re

from vbz_compression_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vbz_gpu_pack_batch", "vbz_gpu_decompressed_size_batch")


def test_exported_and_declared():
    L = _lib.load()
    text = open(os.path.join(ROOT, "include", "vbz_gpu.h")).read()
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in _lib.GPU_API
        assert re.search(r"VBZ_EXPORT\s+int\s+" + n + r"\s*\(", text), n


def test_null_context_is_minus_one():
    L = _lib.load()
    b = _lib.GpuBatch()
    opts = _lib.CompressionOptions(True, 2, 1, 1)
    off = (ctypes.c_uint64 * 2)()
    size = (ctypes.c_uint32 * 1)()
    assert L.vbz_gpu_pack_batch(None, ctypes.byref(b), 16, None, 0, ctypes.addressof(off), ctypes.addressof(size)) == -1
    assert L.vbz_gpu_decompressed_size_batch(None, ctypes.byref(b), ctypes.byref(opts), 16, ctypes.addressof(size), ctypes.addressof(off)) == -1
    assert L.vbz_gpu_pack_batch(None, None, 16, None, 0, None, None) == -1
    assert L.vbz_gpu_decompressed_size_batch(None, None, None, 16, None, None) == -1
