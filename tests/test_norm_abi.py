"""CPU tests of the normalising decode's entry points (include/vbz_gpu.h: vbz_gpu_signal_norm_batch,
vbz_gpu_decompress_signal_norm_batch, vbz_gpu_decompress_chunks_norm_batch): exported, declared with their struct and macros, and
refused without a context before anything touches a device."""
import ctypes
import os
import re

from vbz_compression_amd import _lib, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vbz_gpu_signal_norm_batch", "vbz_gpu_decompress_signal_norm_batch", "vbz_gpu_decompress_chunks_norm_batch")


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
    for macro, value in (("VBZ_GPU_NORM_MED_MAD", 1), ("VBZ_GPU_NORM_QUANTILE", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), text), macro
        assert getattr(_lib, macro) == value
    assert ctypes.sizeof(_lib.GpuNormalization) == 32
    fields = re.search(r"typedef struct vbz_gpu_normalization\s*\{(.*?)\}\s*vbz_gpu_normalization;", text, re.S).group(1)
    names = re.findall(r"^\s*(?:uint32_t|float)\s+(\w+)(?:,\s*(\w+))?;", fields, re.M)
    flat = [n for pair in names for n in pair if n]
    assert flat == [f[0] for f in _lib.GpuNormalization._fields_]


def test_presets():
    m = batch.MED_MAD.c_struct()
    assert (m.method, m.reserved, m.quantile_a, m.quantile_b, m.shift_mul, m.shift_min) == (1, 0, 0.0, 0.0, 1.0, float("-inf"))
    assert abs(m.scale_mul - 1.4826) < 1e-6 and m.scale_min == batch.FLT_MIN
    d = batch.DORADO_QUANTILE.c_struct()
    assert d.method == 2 and (d.shift_min, d.scale_min) == (10.0, 1.0)
    assert abs(d.quantile_a - 0.2) < 1e-7 and abs(d.quantile_b - 0.9) < 1e-7 and abs(d.shift_mul - 0.51) < 1e-7 and abs(d.scale_mul - 0.53) < 1e-7


def test_null_context_or_batch_is_minus_one():
    L = _lib.load()
    b = _lib.GpuBatch()
    opts = _lib.CompressionOptions(True, 2, 1, 1)
    f = _lib.GpuSignalFormat()
    f.out_type = _lib.VBZ_GPU_SIGNAL_F16
    f.is_signed = 1
    ch = _lib.GpuChunking()
    ch.chunk_len, ch.step, ch.mode = 16, 8, _lib.VBZ_GPU_CHUNK_PAD
    m = batch.MED_MAD.c_struct()
    for ctx_b in ((None, ctypes.byref(b)), (None, None)):
        assert L.vbz_gpu_signal_norm_batch(*ctx_b, ctypes.byref(opts), 0, 1, ctypes.byref(m), None) == -1
        assert L.vbz_gpu_decompress_signal_norm_batch(*ctx_b, ctypes.byref(opts), 0, ctypes.byref(f), ctypes.byref(m), None) == -1
        assert L.vbz_gpu_decompress_chunks_norm_batch(*ctx_b, ctypes.byref(opts), 0, ctypes.byref(f), ctypes.byref(ch), None, None, 0,
                                                      ctypes.byref(m), None) == -1
    assert L.vbz_gpu_signal_norm_batch(None, None, None, 0, 0, None, None) == -1
