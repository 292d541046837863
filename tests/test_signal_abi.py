"""CPU tests of the calibrated-signal decode entry point (include/vbz_gpu.h: vbz_gpu_decompress_signal_batch): exported, declared with
its format struct, and refused without a context before anything touches a device."""
import ctypes
import os
import re

from vbz_compression_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "vbz_gpu_decompress_signal_batch"


def test_exported_and_declared():
    L = _lib.load()
    text = open(os.path.join(ROOT, "include", "vbz_gpu.h")).read()
    assert hasattr(L, NAME)
    assert NAME in _lib.GPU_API
    assert re.search(r"VBZ_EXPORT\s+int\s+" + NAME + r"\s*\(", text)
    for macro, value in (("VBZ_GPU_SIGNAL_F32", 1), ("VBZ_GPU_SIGNAL_F16", 2), ("VBZ_GPU_SIGNAL_BF16", 3)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), text), macro
        assert getattr(_lib, macro) == value
    assert ctypes.sizeof(_lib.GpuSignalFormat) == 24


def test_null_context_or_batch_is_minus_one():
    L = _lib.load()
    b = _lib.GpuBatch()
    opts = _lib.CompressionOptions(True, 2, 1, 1)
    f = _lib.GpuSignalFormat()
    f.out_type = _lib.VBZ_GPU_SIGNAL_F32
    f.is_signed = 1
    fn = getattr(L, NAME)
    assert fn(None, ctypes.byref(b), ctypes.byref(opts), 0, ctypes.byref(f)) == -1
    assert fn(None, None, ctypes.byref(opts), 1, ctypes.byref(f)) == -1
    assert fn(None, None, None, 0, None) == -1
