"""CPU tests of the signal-event entry points (include/vbz_gpu.h: vbz_gpu_events): exported, declared with their structs, listed in
_lib.GPU_API, and refused without a context before anything touches a device."""
import ctypes
import inspect
import os
import re

from vbz_compression_amd import _lib, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vbz_gpu_signal_events_batch", "vbz_gpu_pod5_signal_events_batch")
SIZE = {"uint32_t": 4, "float": 4, "uint64_t": 8, "int64_t": 8, "int32_t": 4}


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


def layout(name, S, size, offsets):
    """the ctypes struct against the stated size and offsets, and against the header's own fields laid out by the C rules"""
    assert ctypes.sizeof(S) == size
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == offsets
    fields = re.search(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + r";\s*/\* (\d+) bytes \*/", header(), re.S)
    assert fields, name
    assert int(fields.group(2)) == size
    decl = re.findall(r"^\s*(const\s+)?(uint32_t|uint64_t|int64_t|int32_t|float)(\*?)\s+(\w+);", fields.group(1), re.M)
    assert [d[3] for d in decl] == [f[0] for f in S._fields_]
    off = 0
    for (_, ctype, ptr, field) in decl:
        sz = 8 if ptr else SIZE[ctype]
        off = (off + sz - 1) // sz * sz
        assert off == getattr(S, field).offset, (name, field)
        off += sz
    assert off == size


def test_struct_layouts():
    layout("vbz_gpu_events", _lib.GpuEvents, 32, [("event_rows", 0), ("event_first", 8), ("start", 16), ("flags", 24), ("reserved", 28)])
    layout("vbz_gpu_event", _lib.GpuEvent, 16, [("mean", 0), ("sd", 4), ("n", 8), ("zero", 12)])
    layout("vbz_gpu_event_moments", _lib.GpuEventMoments, 16, [("sum", 0), ("sumsq", 8)])


def test_codec_methods():
    for name, first in (("signal_events", "dst_off"), ("pod5_signal_events", "row_samples")):
        p = inspect.signature(getattr(batch.GpuCodec, name)).parameters
        assert {first, "event_first", "start", "scale", "offset", "signed", "norm", "norm_out", "begin", "end", "stats", "moments"} <= set(p), name
    assert {"ev", "moments"} <= set(inspect.signature(batch.GpuCodec._typed).parameters)


def test_null_context_or_batch_is_minus_one():
    L = _lib.load()
    b = _lib.GpuBatch()
    opts = _lib.CompressionOptions(True, 2, 1, 1)
    popts = batch.pod5_options()
    f = _lib.GpuSignalFormat()
    f.out_type = _lib.VBZ_GPU_SIGNAL_F32
    f.is_signed = 1
    ev = _lib.GpuEvents()
    r = _lib.GpuPod5Reads()
    g = _lib.GpuSampleRanges()
    for ctx_b in ((None, ctypes.byref(b)), (None, None)):
        assert L.vbz_gpu_signal_events_batch(*ctx_b, ctypes.byref(opts), 0, ctypes.byref(f), ctypes.byref(ev), None, None, None, None, ctypes.byref(g)) == -1
        assert L.vbz_gpu_pod5_signal_events_batch(*ctx_b, ctypes.byref(popts), ctypes.byref(f), ctypes.byref(r), ctypes.byref(ev), None, None, None, None,
                                                  ctypes.byref(g)) == -1
