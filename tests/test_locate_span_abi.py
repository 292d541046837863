"""CPU tests of the locate span entry points (include/vbz_gpu.h: vbz_gpu_locate_span_batch and its two fused twins): exported, declared
with their locate twins' arguments and the 16-byte hit of the match span calls, listed in _lib.GPU_API, the struct they share with the
locate calls tied to the header, and refused without a context before anything touches a device."""
import ctypes
import inspect
import re

from test_locate_abi import SIZE, header, prototype
from vbz_compression_amd import _lib, batch

NAMES = ("vbz_gpu_locate_span_batch", "vbz_gpu_signal_locate_span_batch", "vbz_gpu_pod5_signal_locate_span_batch")


def test_exported_declared_and_listed():
    L = _lib.load()
    text = header()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in _lib.GPU_API, name
        assert getattr(L, name).restype == ctypes.c_int and getattr(L, name).argtypes, name
        twin = name.replace("_span", "")
        # the header's prototype is the locate twin's with the hit exchanged -- and the match span twin's with the struct exchanged
        assert prototype(text, name) == [a.replace("vbz_gpu_match_hit*", "vbz_gpu_match_span*") for a in prototype(text, twin)], name
        assert prototype(text, name) == [a.replace("vbz_gpu_match*", "vbz_gpu_locate*") for a in prototype(text, name.replace("_locate", "_match"))], name
        assert list(getattr(L, name).argtypes) == list(getattr(L, twin).argtypes), name
    assert [len(getattr(L, name).argtypes) for name in NAMES] == [6, 11, 11]
    assert sum(1 for a in L.vbz_gpu_locate_span_batch.argtypes if a is ctypes.POINTER(_lib.GpuLocate)) == 1
    assert all(prototype(text, name)[-1] == "vbz_gpu_match_span*" for name in NAMES)


def test_the_structs_are_the_twins():
    """the same vbz_gpu_locate (40 bytes, one declaration) and the match span calls' 16-byte record"""
    text = header()
    assert len(re.findall(r"typedef struct vbz_gpu_locate\b", text)) == 1 and len(re.findall(r"typedef struct vbz_gpu_match_span\b", text)) == 1
    fields = re.search(r"typedef struct vbz_gpu_locate\s*\{(.*?)\}\s*vbz_gpu_locate;\s*/\* (\d+) bytes \*/", text, re.S)
    assert fields and int(fields.group(2)) == 40 == ctypes.sizeof(_lib.GpuLocate)
    decl = re.findall(r"^\s*(uint32_t|float|const int8_t\*|const uint32_t\*)\s+(\w+);", fields.group(1), re.M)
    off = 0
    for ctype, field in decl:
        sz = SIZE[ctype]
        off = (off + sz - 1) // sz * sz
        assert off == getattr(_lib.GpuLocate, field).offset, field
        off += sz
    assert off == 40
    span = re.search(r"typedef struct vbz_gpu_match_span\s*\{(.*?)\}\s*vbz_gpu_match_span;\s*/\* (\d+) bytes \*/", text, re.S)
    assert span and int(span.group(2)) == 16 == ctypes.sizeof(_lib.GpuMatchSpan)
    assert re.findall(r"uint32_t\s+(\w+);", span.group(1)) == ["cost", "end", "start", "zero"] == [f[0] for f in _lib.GpuMatchSpan._fields_]
    assert [getattr(_lib.GpuMatchSpan, f).offset for f in ("cost", "end", "start", "zero")] == [0, 4, 8, 12]
    assert text.index("} vbz_gpu_match_span;") < text.index("} vbz_gpu_locate;") < text.index("vbz_gpu_locate_span_batch(")


def test_the_header_states_the_rule():
    text = header()
    text = text[text.index("/* Signal locate with the start") : text.index("VBZ_EXPORT int vbz_gpu_locate_span_batch")]
    for phrase in ("span_brute(levels of the read, target[:L])", "from (0, s) to (n - 1, e - 1)", "(i+1, j)", "(i, j+1), (i+1, j+1)",
                   "horizontal steps inside row 0 count", "the SMALLEST s over all paths of cost `cost` that end at column end - 1",
                   "start < end always", "start <= 2^30 - 1", "{cost, end, start, 0}", "{0xFFFFFFFF, 0, 0, 0}", "n == 0, an empty range",
                   "target_len 0 or above target_stride", "n_reads * G * 16 beyond 2^46 bytes", "flags and reserved", "rows the query, columns the target",
                   "vbz_gpu_match_best_batch(ctx, n_reads, spans, G, max_cost, pairs)", "TARGET coordinates", "No LDS, no barrier"):
        assert phrase in text, phrase
    locate = header()
    locate = locate[locate.index("/* Signal locate.") : locate.index("} vbz_gpu_locate;")]
    assert "Not here: the path" in locate and "the start of the stretch and the path" not in locate


def test_codec_methods():
    p = inspect.signature(batch.GpuCodec.locate_span).parameters
    assert list(p) == [k for k in inspect.signature(batch.GpuCodec.locate).parameters if k != "span"]
    for name in ("signal_locate", "pod5_signal_locate"):
        assert "span" in inspect.signature(getattr(batch.GpuCodec, name)).parameters and callable(getattr(batch.GpuCodec, name + "_span"))
    assert "words" in inspect.signature(batch.GpuCodec._locate_arenas).parameters


def test_null_context_or_batch_is_minus_one():
    L = _lib.load()
    b = _lib.GpuBatch()
    opts = _lib.CompressionOptions(True, 2, 1, 1)
    popts = batch.pod5_options()
    m = _lib.GpuLocate()
    f = _lib.GpuSignalFormat()
    r = _lib.GpuPod5Reads()
    assert L.vbz_gpu_locate_span_batch(None, 0, None, None, ctypes.byref(m), None) == -1
    for ctx_b in ((None, ctypes.byref(b)), (None, None)):
        assert L.vbz_gpu_signal_locate_span_batch(*ctx_b, ctypes.byref(opts), 0, ctypes.byref(f), None, None, None, ctypes.byref(m), None, None) == -1
        assert L.vbz_gpu_pod5_signal_locate_span_batch(*ctx_b, ctypes.byref(popts), ctypes.byref(f), ctypes.byref(r), None, None, None, ctypes.byref(m), None,
                                                       None) == -1
