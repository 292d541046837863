"""CPU tests of the signal-match entry points (include/vbz_gpu.h: vbz_gpu_match): exported, declared with their structs, listed in
_lib.GPU_API, and refused without a context before anything touches a device."""
import ctypes
import inspect
import os
import re

import numpy as np

from vbz_compression_amd import _lib, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vbz_gpu_match_batch", "vbz_gpu_signal_match_batch", "vbz_gpu_pod5_signal_match_batch")
SIZE = {"uint32_t": 4, "float": 4, "const int8_t*": 8, "const uint32_t*": 8}


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
    assert [len(getattr(L, name).argtypes) for name in NAMES] == [6, 11, 11]


def laid_out(struct, name, size):
    """the ctypes struct against the header's own fields laid out by the C rules"""
    fields = re.search(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + r";\s*/\* (\d+) bytes \*/", header(), re.S)
    assert fields and int(fields.group(2)) == size == ctypes.sizeof(struct), name
    decl = re.findall(r"^\s*(uint32_t|float|const int8_t\*|const uint32_t\*)\s+(\w+);", fields.group(1), re.M)
    assert [d[1] for d in decl] == [f[0] for f in struct._fields_], name
    off = 0
    for ctype, field in decl:
        sz = SIZE[ctype]
        off = (off + sz - 1) // sz * sz
        assert off == getattr(struct, field).offset, field
        off += sz
    assert off == size


def test_struct_layout():
    S = _lib.GpuMatch
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("query_len", 0), ("n_refs", 4), ("ref_stride", 8), ("flags", 12), ("quant", 16),
                                                                   ("reserved", 20), ("ref", 24), ("ref_len", 32)]
    laid_out(S, "vbz_gpu_match", 40)
    H = _lib.GpuMatchHit
    assert [(n, getattr(H, n).offset) for n, _ in H._fields_] == [("cost", 0), ("end", 4)]
    laid_out(H, "vbz_gpu_match_hit", 8)


def test_the_header_states_the_rule():
    text = header()
    for phrase in ("n = min(T', N)", "clamp(rint(v), -127, 127)", "k_j = 0 when v is NaN", "D[0][j] = c(0, j)", "D[i][0] = c(i, 0) + D[i-1][0]",
                   "min(D[i-1][j-1], D[i-1][j], D[i][j-1])", "the SMALLEST j that attains it", "D[i][j] <= 255 (i + 1) < 2^20", "{0xFFFFFFFF, 0}",
                   "no address is formed from it", "EVERY entry is written", "-128 is legal", "query is REQUIRED", "a bad first_row fails the whole call"):
        assert phrase in text, phrase


def test_codec_methods():
    p = inspect.signature(batch.GpuCodec.match).parameters
    assert {"query", "valid", "ref", "ref_len", "match", "out"} <= set(p)
    for name, first in (("signal_match", "dst_off"), ("pod5_signal_match", "row_samples")):
        p = inspect.signature(getattr(batch.GpuCodec, name)).parameters
        assert {first, "ref", "ref_len", "match", "scale", "offset", "signed", "norm", "norm_out", "begin", "end", "stats", "query", "out"} <= set(p), name
    assert "sized" in inspect.signature(batch.GpuCodec.signal_match).parameters
    assert "read_result" in inspect.signature(batch.GpuCodec.pod5_signal_match).parameters
    assert "mt" in inspect.signature(batch.GpuCodec._typed).parameters
    assert {f.name for f in batch.Match.__dataclass_fields__.values()} == {"query_len", "quant"}
    assert (batch.Match().query_len, batch.Match().quant) == (2048, 32.0)
    assert batch.quantize_levels(np.array([0.5, 1.5, np.nan, np.inf, -9.0], np.float32), 32.0).tolist() == [16, 48, 0, 127, -127]


def test_null_context_or_batch_is_minus_one():
    L = _lib.load()
    b = _lib.GpuBatch()
    opts = _lib.CompressionOptions(True, 2, 1, 1)
    popts = batch.pod5_options()
    m = _lib.GpuMatch()
    f = _lib.GpuSignalFormat()
    r = _lib.GpuPod5Reads()
    assert L.vbz_gpu_match_batch(None, 0, None, None, ctypes.byref(m), None) == -1
    for ctx_b in ((None, ctypes.byref(b)), (None, None)):
        assert L.vbz_gpu_signal_match_batch(*ctx_b, ctypes.byref(opts), 0, ctypes.byref(f), None, None, None, ctypes.byref(m), None, None) == -1
        assert L.vbz_gpu_pod5_signal_match_batch(*ctx_b, ctypes.byref(popts), ctypes.byref(f), ctypes.byref(r), None, None, None, ctypes.byref(m), None, None) == -1
