"""CPU tests of the signal-segmentation entry points (include/vbz_gpu.h: vbz_gpu_segmentation): exported, declared with their struct,
listed in _lib.GPU_API, and refused without a context before anything touches a device."""
import ctypes
import inspect
import os
import re

from vbz_compression_amd import _lib, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vbz_gpu_signal_segment_batch", "vbz_gpu_pod5_signal_segment_batch")
SIZE = {"uint32_t": 4, "float": 4, "uint64_t": 8}


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
    """the ctypes struct against the stated size and offsets, and against the header's own fields laid out by the C rules"""
    S, size = _lib.GpuSegmentation, 32
    assert ctypes.sizeof(S) == size
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("short_window", 0), ("long_window", 4), ("short_threshold", 8), ("long_threshold", 12),
                                                                   ("radius", 16), ("flags", 20), ("start_cap", 24)]
    fields = re.search(r"typedef struct vbz_gpu_segmentation\s*\{(.*?)\}\s*vbz_gpu_segmentation;\s*/\* (\d+) bytes \*/", header(), re.S)
    assert fields and int(fields.group(2)) == size
    decl = re.findall(r"^\s*(uint32_t|uint64_t|float)\s+(\w+);", fields.group(1), re.M)
    assert [d[1] for d in decl] == [f[0] for f in S._fields_]
    off = 0
    for ctype, field in decl:
        sz = SIZE[ctype]
        off = (off + sz - 1) // sz * sz
        assert off == getattr(S, field).offset, field
        off += sz
    assert off == size


def test_the_header_states_the_rule():
    text = header()
    for phrase in ("rows <= 2 + T' / (r + 1)", "Of equal scores the first wins", "D = max(w (A2 + B2) - A^2 - B^2, 1)", "count-only call"):
        assert phrase in text, phrase


def test_codec_methods():
    for name, first in (("signal_segment", "dst_off"), ("pod5_signal_segment", "row_samples")):
        p = inspect.signature(getattr(batch.GpuCodec, name)).parameters
        assert {first, "segmentation", "start_cap", "signed", "begin", "end", "event_first", "start"} <= set(p), name
        assert not {"scale", "offset", "norm", "stats"} & set(p), name   # (the score does not change under offset and scale)
    assert "sized" in inspect.signature(batch.GpuCodec.signal_segment).parameters
    assert "read_result" in inspect.signature(batch.GpuCodec.pod5_signal_segment).parameters
    assert {"sg", "event_first", "start"} <= set(inspect.signature(batch.GpuCodec._typed).parameters)
    g = batch.Segmentation(3, 6, 4.0, 9.0, 2).c_struct(77)
    assert (g.short_window, g.long_window, g.short_threshold, g.long_threshold, g.radius, g.flags, g.start_cap) == (3, 6, 4.0, 9.0, 2, 0, 77)
    assert batch.Segmentation(radius=2).max_rows(10) == 5


def test_null_context_or_batch_is_minus_one():
    L = _lib.load()
    b = _lib.GpuBatch()
    opts = _lib.CompressionOptions(True, 2, 1, 1)
    popts = batch.pod5_options()
    sg = batch.Segmentation().c_struct()
    r = _lib.GpuPod5Reads()
    g = _lib.GpuSampleRanges()
    for ctx_b in ((None, ctypes.byref(b)), (None, None)):
        assert L.vbz_gpu_signal_segment_batch(*ctx_b, ctypes.byref(opts), 0, 1, ctypes.byref(g), ctypes.byref(sg), None, None) == -1
        assert L.vbz_gpu_pod5_signal_segment_batch(*ctx_b, ctypes.byref(popts), 1, ctypes.byref(r), ctypes.byref(g), ctypes.byref(sg), None, None) == -1
