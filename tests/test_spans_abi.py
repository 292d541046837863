"""CPU tests of the signal-span entry points (include/vbz_gpu.h: vbz_gpu_spans): exported, declared with their struct, listed in
_lib.GPU_API, and refused without a context before anything touches a device."""
import ctypes
import inspect
import os
import re

from vbz_compression_amd import _lib, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vbz_gpu_signal_spans_batch", "vbz_gpu_pod5_signal_spans_batch")
SIZE = {"uint32_t": 4, "float": 4, "uint64_t": 8, "const float*": 8}


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
    assert len(L.vbz_gpu_signal_spans_batch.argtypes) == 11 and len(L.vbz_gpu_pod5_signal_spans_batch.argtypes) == 11


def test_struct_layout():
    """the ctypes struct against the stated size and offsets, and against the header's own fields laid out by the C rules"""
    S, size = _lib.GpuSpans, 40
    assert ctypes.sizeof(S) == size
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("direction", 0), ("merge_gap", 4), ("min_length", 8), ("ignore_prefix", 12),
                                                                   ("threshold_factor", 16), ("flags", 20), ("level", 24), ("edge_cap", 32)]
    fields = re.search(r"typedef struct vbz_gpu_spans\s*\{(.*?)\}\s*vbz_gpu_spans;\s*/\* (\d+) bytes \*/", header(), re.S)
    assert fields and int(fields.group(2)) == size
    decl = re.findall(r"^\s*(uint32_t|uint64_t|float|const float\*)\s+(\w+);", fields.group(1), re.M)
    assert [d[1] for d in decl] == [f[0] for f in S._fields_]
    off = 0
    for ctype, field in decl:
        sz = SIZE[ctype]
        off = (off + sz - 1) // sz * sz
        assert off == getattr(S, field).offset, field
        off += sz
    assert off == size
    text = header()
    assert re.search(r"#define VBZ_GPU_SPAN_ABOVE 0u", text) and re.search(r"#define VBZ_GPU_SPAN_BELOW 1u", text)
    assert (_lib.VBZ_GPU_SPAN_ABOVE, _lib.VBZ_GPU_SPAN_BELOW) == (0, 1)


def test_the_header_states_the_rule():
    text = header()
    for phrase in ("spans <= (T' + D + 1) / (m + D + 1)", "a sample equal to thr is not in", "q' - q - 1 <= D", "the length test comes after the merge",
                   "count-only call", "one multiply, then one add", "A NaN thr makes nothing in", "not one word of edge"):
        assert phrase in text, phrase


def test_codec_methods():
    for name, first in (("signal_spans", "dst_off"), ("pod5_signal_spans", "row_samples")):
        p = inspect.signature(getattr(batch.GpuCodec, name)).parameters
        assert {first, "spans", "edge_cap", "signed", "begin", "end", "edge_first", "edge", "norm", "level", "shift_scale", "stats"} <= set(p), name
    assert "sized" in inspect.signature(batch.GpuCodec.signal_spans).parameters
    assert "read_result" in inspect.signature(batch.GpuCodec.pod5_signal_spans).parameters
    typed = set(inspect.signature(batch.GpuCodec._typed).parameters)
    assert {"sp", "sg", "event_first", "start", "m", "ss", "g", "r", "t", "out", "w", "ev", "moments", "ch", "chunk_first", "chunks", "f"} <= typed
    g = batch.Spans("below", 50, 5, 7, 2.5).c_struct(77, 4096)
    assert (g.direction, g.merge_gap, g.min_length, g.ignore_prefix, g.threshold_factor, g.flags, g.level, g.edge_cap) == (1, 50, 5, 7, 2.5, 0, 4096, 77)
    assert batch.Spans().c_struct().direction == 0 and batch.Spans("sideways").c_struct().direction == 0xFFFFFFFF
    assert batch.Spans(merge_gap=50, min_length=5).max_edges(100_000) == 2 * ((100_000 + 51) // 56)
    assert batch.Spans(merge_gap=9, min_length=3).max_edges(0) == 0


def test_null_context_or_batch_is_minus_one():
    L = _lib.load()
    b = _lib.GpuBatch()
    opts = _lib.CompressionOptions(True, 2, 1, 1)
    popts = batch.pod5_options()
    sp = batch.Spans().c_struct()
    r = _lib.GpuPod5Reads()
    g = _lib.GpuSampleRanges()
    for ctx_b in ((None, ctypes.byref(b)), (None, None)):
        assert L.vbz_gpu_signal_spans_batch(*ctx_b, ctypes.byref(opts), 0, 1, None, None, ctypes.byref(g), ctypes.byref(sp), None, None) == -1
        assert L.vbz_gpu_pod5_signal_spans_batch(*ctx_b, ctypes.byref(popts), 1, ctypes.byref(r), None, None, ctypes.byref(g), ctypes.byref(sp), None, None) == -1
