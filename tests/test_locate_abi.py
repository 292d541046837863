"""CPU tests of the signal-locate entry points (include/vbz_gpu.h: vbz_gpu_locate): exported, declared with their struct, listed in
_lib.GPU_API with their match twins' arguments, and refused without a context before anything touches a device."""
import ctypes
import inspect
import os
import re

from vbz_compression_amd import _lib, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vbz_gpu_locate_batch", "vbz_gpu_signal_locate_batch", "vbz_gpu_pod5_signal_locate_batch")
SIZE = {"uint32_t": 4, "float": 4, "const int8_t*": 8, "const uint32_t*": 8}


def header():
    return open(os.path.join(ROOT, "include", "vbz_gpu.h")).read()


def prototype(text, name):
    """the argument types of a declaration, names and spaces dropped"""
    m = re.search(r"VBZ_EXPORT\s+int\s+" + name + r"\s*\((.*?)\);", text, re.S)
    assert m, name
    return [re.sub(r"\s*\w+$", "", " ".join(a.split())) for a in m.group(1).split(",")]


def test_exported_declared_and_listed():
    L = _lib.load()
    text = header()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in _lib.GPU_API, name
        assert getattr(L, name).restype == ctypes.c_int and getattr(L, name).argtypes, name
        twin = name.replace("_locate", "_match")
        # the header's prototype is the twin's with the struct exchanged
        assert prototype(text, name) == [a.replace("vbz_gpu_match*", "vbz_gpu_locate*") for a in prototype(text, twin)], name
        want = [ctypes.POINTER(_lib.GpuLocate) if a is ctypes.POINTER(_lib.GpuMatch) else a for a in getattr(L, twin).argtypes]
        assert list(getattr(L, name).argtypes) == want, name
    assert [len(getattr(L, name).argtypes) for name in NAMES] == [6, 11, 11]
    assert sum(1 for a in L.vbz_gpu_locate_batch.argtypes if a is ctypes.POINTER(_lib.GpuLocate)) == 1


def test_struct_layout():
    S = _lib.GpuLocate
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("query_len", 0), ("n_targets", 4), ("target_stride", 8), ("flags", 12), ("quant", 16),
                                                                   ("reserved", 20), ("target", 24), ("target_len", 32)]
    fields = re.search(r"typedef struct vbz_gpu_locate\s*\{(.*?)\}\s*vbz_gpu_locate;\s*/\* (\d+) bytes \*/", header(), re.S)
    assert fields and int(fields.group(2)) == 40 == ctypes.sizeof(S)
    decl = re.findall(r"^\s*(uint32_t|float|const int8_t\*|const uint32_t\*)\s+(\w+);", fields.group(1), re.M)
    assert [d[1] for d in decl] == [f[0] for f in S._fields_]
    off = 0
    for ctype, field in decl:
        sz = SIZE[ctype]
        off = (off + sz - 1) // sz * sz
        assert off == getattr(S, field).offset, field
        off += sz
    assert off == 40


def test_the_header_states_the_rule():
    text = header()
    text = text[text.index("/* Signal locate.") : text.index("} vbz_gpu_locate;")]
    for phrase in ("n = min(T', N)", "NaN -> 0, clamp to +-127, rint to nearest even", "D[0][j] = c(0, j)", "D[i][0] = c(i, 0) + D[i-1][0]",
                   "min(D[i-1][j-1], D[i-1][j], D[i][j-1])", "the SMALLEST j that attains it", "D <= 255 n < 2^20", "end <= 2^30", "{0xFFFFFFFF, 0}",
                   "no address is formed from it", "Every entry is written", "-128 is legal", "REQUIRED query", "rows the query, columns the target",
                   "a multiple of 8, 8 ... 2048", "a multiple of 16, 16 ... 2^30", "G: 1 ... 4096"):
        assert phrase in text, phrase


def test_codec_methods():
    p = inspect.signature(batch.GpuCodec.locate).parameters
    assert {"query", "valid", "target", "target_len", "locate", "out"} <= set(p)
    for name, first in (("signal_locate", "dst_off"), ("pod5_signal_locate", "row_samples")):
        p = inspect.signature(getattr(batch.GpuCodec, name)).parameters
        assert {first, "target", "target_len", "locate", "scale", "offset", "signed", "norm", "norm_out", "begin", "end", "stats", "query", "out"} <= set(p), name
    assert "sized" in inspect.signature(batch.GpuCodec.signal_locate).parameters
    assert "read_result" in inspect.signature(batch.GpuCodec.pod5_signal_locate).parameters
    assert "lc" in inspect.signature(batch.GpuCodec._typed).parameters
    assert {f.name for f in batch.Locate.__dataclass_fields__.values()} == {"query_len", "quant"}
    assert (batch.Locate().query_len, batch.Locate().quant) == (2048, 32.0)


def test_null_context_or_batch_is_minus_one():
    L = _lib.load()
    b = _lib.GpuBatch()
    opts = _lib.CompressionOptions(True, 2, 1, 1)
    popts = batch.pod5_options()
    m = _lib.GpuLocate()
    f = _lib.GpuSignalFormat()
    r = _lib.GpuPod5Reads()
    assert L.vbz_gpu_locate_batch(None, 0, None, None, ctypes.byref(m), None) == -1
    for ctx_b in ((None, ctypes.byref(b)), (None, None)):
        assert L.vbz_gpu_signal_locate_batch(*ctx_b, ctypes.byref(opts), 0, ctypes.byref(f), None, None, None, ctypes.byref(m), None, None) == -1
        assert L.vbz_gpu_pod5_signal_locate_batch(*ctx_b, ctypes.byref(popts), ctypes.byref(f), ctypes.byref(r), None, None, None, ctypes.byref(m), None, None) == -1
