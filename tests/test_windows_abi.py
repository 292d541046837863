"""CPU tests of the signal-window entry points (include/vbz_gpu.h: vbz_gpu_windows): exported, declared with their struct, listed in
_lib.GPU_API, and refused without a context before anything touches a device."""
import ctypes
import inspect
import os
import re

from vbz_compression_amd import _lib, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vbz_gpu_decompress_windows_batch", "vbz_gpu_pod5_decompress_windows_batch")


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
    S = _lib.GpuWindows
    assert ctypes.sizeof(S) == 40
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("window_len", 0), ("pad", 4), ("window_rows", 8), ("window_first", 16), ("start", 24),
                                                                  ("flags", 32), ("reserved", 36)]
    fields = re.search(r"typedef struct vbz_gpu_windows\s*\{(.*?)\}\s*vbz_gpu_windows;\s*/\* (\d+) bytes \*/", text, re.S)
    assert int(fields.group(2)) == 40
    decl = re.findall(r"^\s*(const\s+)?(uint32_t|uint64_t|int32_t|float)(\*?)\s+(\w+);", fields.group(1), re.M)
    assert [d[3] for d in decl] == [f[0] for f in S._fields_]
    size = {"uint32_t": 4, "float": 4, "uint64_t": 8, "int32_t": 4}
    off = 0
    for (_, ctype, ptr, name) in decl:   # the header's own fields, laid out by the C rules, land where ctypes puts them
        sz = 8 if ptr else size[ctype]
        off = (off + sz - 1) // sz * sz
        assert off == getattr(S, name).offset, name
        off += sz
    assert off == 40


def test_codec_methods():
    for name, first in (("decompress_windows", "samples"), ("pod5_decompress_windows", "row_samples")):
        p = inspect.signature(getattr(batch.GpuCodec, name)).parameters
        assert {first, "window_first", "start", "window_len", "pad", "dtype", "scale", "offset", "signed", "norm", "norm_out", "begin", "end", "stats"} <= set(p), name
    assert "w" in inspect.signature(batch.GpuCodec._typed).parameters


def test_null_context_or_batch_is_minus_one():
    L = _lib.load()
    b = _lib.GpuBatch()
    opts = _lib.CompressionOptions(True, 2, 1, 1)
    popts = batch.pod5_options()
    f = _lib.GpuSignalFormat()
    f.out_type = _lib.VBZ_GPU_SIGNAL_F16
    f.is_signed = 1
    w = _lib.GpuWindows()
    w.window_len = 16
    r = _lib.GpuPod5Reads()
    g = _lib.GpuSampleRanges()
    for ctx_b in ((None, ctypes.byref(b)), (None, None)):
        assert L.vbz_gpu_decompress_windows_batch(*ctx_b, ctypes.byref(opts), 0, ctypes.byref(f), ctypes.byref(w), None, None, None, ctypes.byref(g)) == -1
        assert L.vbz_gpu_pod5_decompress_windows_batch(*ctx_b, ctypes.byref(popts), ctypes.byref(f), ctypes.byref(r), ctypes.byref(w), None, None, None,
                                                       ctypes.byref(g)) == -1
