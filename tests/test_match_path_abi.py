"""CPU tests of the path entry points (include/vbz_gpu.h: vbz_gpu_match_best_batch, vbz_gpu_match_path_batch,
vbz_gpu_set_match_path_cap): exported by the built library, declared with their structs, listed in _lib.GPU_API, the ctypes structs tied
to the header's fields, refused without a context before anything touches a device; vbz_gpu_match_span as it was."""
import ctypes
import inspect
import os
import re

from vbz_compression_amd import _lib, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vbz_gpu_match_best_batch", "vbz_gpu_match_path_batch", "vbz_gpu_set_match_path_cap")
U32, U64 = ctypes.c_uint32, ctypes.c_uint64


def header():
    return open(os.path.join(ROOT, "include", "vbz_gpu.h")).read()


def test_exported_declared_and_listed():
    L = _lib.load()
    text = header()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in _lib.GPU_API, name
        assert re.search(r"VBZ_EXPORT\s+(int|void)\s+" + name + r"\s*\(", text), name
    vp = ctypes.c_void_p
    assert L.vbz_gpu_match_best_batch.restype == ctypes.c_int and L.vbz_gpu_match_best_batch.argtypes == [vp, U32, vp, U32, U32, vp]
    assert L.vbz_gpu_match_path_batch.restype == ctypes.c_int
    assert L.vbz_gpu_match_path_batch.argtypes == [vp, U32, U32, vp, vp, ctypes.POINTER(_lib.GpuMatch), vp, ctypes.POINTER(_lib.GpuMatchPath), vp, vp]
    assert L.vbz_gpu_set_match_path_cap.restype is None and L.vbz_gpu_set_match_path_cap.argtypes == [vp, U64]
    # the header's argument lists, type by type
    args = {n: [re.sub(r"\s+", " ", a).strip() for a in re.search(r"VBZ_EXPORT\s+\w+\s+" + n + r"\s*\((.*?)\);", text, re.S).group(1).split(",")] for n in NAMES}
    assert args[NAMES[0]] == ["vbz_gpu_ctx* ctx", "uint32_t n_reads", "const vbz_gpu_match_span* spans", "uint32_t n_refs", "uint32_t max_cost",
                              "vbz_gpu_match_pair* pairs"]
    assert args[NAMES[1]] == ["vbz_gpu_ctx* ctx", "uint32_t n_pairs", "uint32_t n_reads", "const float* query", "const uint32_t* valid",
                              "const vbz_gpu_match* match", "const vbz_gpu_match_pair* pairs", "const vbz_gpu_match_path* path", "vbz_gpu_match_span* hit",
                              "vbz_gpu_match_row* rows"]
    assert args[NAMES[2]] == ["vbz_gpu_ctx* ctx", "uint64_t bytes"]


def fields_of(name):
    m = re.search(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + r";\s*/\* (\d+) bytes \*/", header(), re.S)
    assert m, name
    return re.findall(r"^\s*(\w+)\s+(\w+);", m.group(1), re.M), int(m.group(2))


def test_struct_layouts():
    ctype = {"uint32_t": U32, "uint64_t": U64}
    for S, name, size, offsets in ((_lib.GpuMatchPair, "vbz_gpu_match_pair", 16, [0, 4, 8, 12]), (_lib.GpuMatchPath, "vbz_gpu_match_path", 16, [0, 4, 8]),
                                   (_lib.GpuMatchRow, "vbz_gpu_match_row", 8, [0, 4])):
        decl, stated = fields_of(name)
        assert ctypes.sizeof(S) == size == stated, name
        assert [(n, t) for n, t in S._fields_] == [(n, ctype[t]) for t, n in decl], name
        assert [getattr(S, n).offset for n, _ in S._fields_] == offsets, name
    assert [n for _, n in fields_of("vbz_gpu_match_pair")[0]] == ["read", "ref", "begin", "end"]
    assert [n for _, n in fields_of("vbz_gpu_match_path")[0]] == ["max_width", "flags", "reserved"]
    assert [n for _, n in fields_of("vbz_gpu_match_row")[0]] == ["begin", "end"]
    # the hit is vbz_gpu_match_span, as it was
    assert ctypes.sizeof(_lib.GpuMatchSpan) == 16 and [n for n, _ in _lib.GpuMatchSpan._fields_] == ["cost", "end", "start", "zero"]


def test_the_header_states_the_rule():
    text = header()
    for phrase in ("a window [a, b) of the read's query", "row 0 at column a is (c(0, a), a)", "step to the FIRST of diagonal (i-1, j-1), up (i-1, j), left (i, j-1)",
                   "at j == a, i > 0:", "step left while j > a and P[0][j-1].cost == 0", "begin_0 == start", "end_{M-1} == b", "begin_{i+1} is end_i - 1",
                   "`zero`, carries rows HERE", "{0xFFFFFFFF, 0, 0, 0} with every row {0, 0}", "ties to the smallest reference index",
                   "ref = 0xFFFFFFFF and begin = end = 0", "valid may be NULL", "a multiple of 8 from 8 to 65536", "EVERY entry of hit and rows is written",
                   "n_pairs * ref_stride * 8 beyond 2^46", "VBZ_HIP_MATCH_PATH_CAP"):
        assert phrase in text, phrase


def test_codec_methods():
    assert list(inspect.signature(batch.GpuCodec.match_best).parameters) == ["self", "spans", "max_cost", "out"]
    assert list(inspect.signature(batch.GpuCodec.match_path).parameters) == ["self", "query", "valid", "ref", "ref_len", "pairs", "max_width", "match", "hit",
                                                                            "rows"]


def test_null_context_is_minus_one():
    L = _lib.load()
    m, p = _lib.GpuMatch(), _lib.GpuMatchPath()
    assert L.vbz_gpu_match_best_batch(None, 0, None, 1, 0, None) == -1
    assert L.vbz_gpu_match_path_batch(None, 0, 0, None, None, ctypes.byref(m), None, ctypes.byref(p), None, None) == -1
    L.vbz_gpu_set_match_path_cap(None, 1 << 20)   # (no context: nothing to set, nothing to touch)
