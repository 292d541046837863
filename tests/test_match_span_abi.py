"""CPU tests of the span entry points (include/vbz_gpu.h: vbz_gpu_match_span): exported, declared with their struct, listed in
_lib.GPU_API with their twins' arguments, refused without a context before anything touches a device; vbz_gpu_match as it was."""
import ctypes
import inspect
import os
import re

from vbz_compression_amd import _lib, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vbz_gpu_match_span_batch", "vbz_gpu_signal_match_span_batch", "vbz_gpu_pod5_signal_match_span_batch")


def header():
    return open(os.path.join(ROOT, "include", "vbz_gpu.h")).read()


def test_exported_declared_and_listed():
    L = _lib.load()
    text = header()
    for name in NAMES:
        twin = name.replace("_span", "")
        assert hasattr(L, name), name
        assert name in _lib.GPU_API, name
        assert re.search(r"VBZ_EXPORT\s+int\s+" + name + r"\s*\(", text), name
        assert getattr(L, name).restype == ctypes.c_int and getattr(L, name).argtypes == getattr(L, twin).argtypes, name
        # the header's argument list is the twin's, the hit type apart
        args = [re.sub(r"\s+", " ", re.search(r"VBZ_EXPORT\s+int\s+" + n + r"\s*\((.*?)\);", text, re.S).group(1)) for n in (name, twin)]
        assert args[0] == args[1].replace("vbz_gpu_match_hit* out", "vbz_gpu_match_span* out"), name
    assert [len(getattr(L, name).argtypes) for name in NAMES] == [6, 11, 11]


def test_struct_layout():
    S = _lib.GpuMatchSpan
    assert ctypes.sizeof(S) == 16
    assert [(n, getattr(S, n).offset, t) for n, t in S._fields_] == [("cost", 0, ctypes.c_uint32), ("end", 4, ctypes.c_uint32),
                                                                      ("start", 8, ctypes.c_uint32), ("zero", 12, ctypes.c_uint32)]
    fields = re.search(r"typedef struct vbz_gpu_match_span\s*\{(.*?)\}\s*vbz_gpu_match_span;\s*/\* (\d+) bytes \*/", header(), re.S)
    assert fields and int(fields.group(2)) == 16
    decl = re.findall(r"^\s*(\w+)\s+(\w+);", fields.group(1), re.M)
    assert decl == [("uint32_t", "cost"), ("uint32_t", "end"), ("uint32_t", "start"), ("uint32_t", "zero")]   # four words: offsets 0 / 4 / 8 / 12
    # the match itself is as it was
    assert ctypes.sizeof(_lib.GpuMatch) == 40 and ctypes.sizeof(_lib.GpuMatchHit) == 8
    assert re.search(r"\}\s*vbz_gpu_match;\s*/\* 40 bytes \*/", header())


def test_the_header_states_the_rule():
    text = header()
    for phrase in ("a path may sit on row 0 for several samples", "start = the SMALLEST s over all paths of cost `cost` that end at column end - 1",
                   "[start, end); start < end always", "P[0][j] = (c(0, j), j)", "if P[0][j-1].cost == 0",
                   "lexmin(P[i-1][j-1], P[i-1][j], P[i][j-1])", "{0xFFFFFFFF, 0, 0, 0}", "n_reads * R * 16", "EVERY entry is written",
                   "255 ref_stride < 2^(31 - sb)", "from query_len and ref_stride alone"):
        assert phrase in text, phrase


def test_codec_methods():
    for name in ("match_span", "signal_match_span", "pod5_signal_match_span"):
        assert callable(getattr(batch.GpuCodec, name)), name
    assert {"query", "valid", "ref", "ref_len", "match", "out"} <= set(inspect.signature(batch.GpuCodec.match_span).parameters)
    assert "span" in inspect.signature(batch.GpuCodec._typed).parameters


def test_null_context_or_batch_is_minus_one():
    L = _lib.load()
    b = _lib.GpuBatch()
    opts = _lib.CompressionOptions(True, 2, 1, 1)
    popts = batch.pod5_options()
    m = _lib.GpuMatch()
    f = _lib.GpuSignalFormat()
    r = _lib.GpuPod5Reads()
    assert L.vbz_gpu_match_span_batch(None, 0, None, None, ctypes.byref(m), None) == -1
    for ctx_b in ((None, ctypes.byref(b)), (None, None)):
        assert L.vbz_gpu_signal_match_span_batch(*ctx_b, ctypes.byref(opts), 0, ctypes.byref(f), None, None, None, ctypes.byref(m), None, None) == -1
        assert L.vbz_gpu_pod5_signal_match_span_batch(*ctx_b, ctypes.byref(popts), ctypes.byref(f), ctypes.byref(r), None, None, None, ctypes.byref(m), None,
                                                      None) == -1
