"""CPU tests of the locate path entry points (include/vbz_gpu.h: vbz_gpu_locate_path_batch, vbz_gpu_query_valid_batch): exported, declared
with the match path call's arguments and a vbz_gpu_locate in vbz_gpu_match's place, listed in _lib.GPU_API, no struct of their own -- the
pair, path, row and span records of the match path, tied to the header -- and refused without a context before anything touches a device."""
import ctypes
import inspect
import re

from test_locate_abi import header, prototype
from vbz_compression_amd import _lib, batch

NAMES = ("vbz_gpu_locate_path_batch", "vbz_gpu_query_valid_batch")


def test_exported_declared_and_listed():
    L = _lib.load()
    text = header()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in _lib.GPU_API, name
        assert getattr(L, name).restype == ctypes.c_int and getattr(L, name).argtypes, name
    # the header's prototype is the match path call's with the struct exchanged
    assert prototype(text, NAMES[0]) == [a.replace("vbz_gpu_match*", "vbz_gpu_locate*") for a in prototype(text, "vbz_gpu_match_path_batch")]
    assert prototype(text, NAMES[0]) == ["vbz_gpu_ctx*", "uint32_t", "uint32_t", "const float*", "const uint32_t*", "const vbz_gpu_locate*",
                                         "const vbz_gpu_match_pair*", "const vbz_gpu_match_path*", "vbz_gpu_match_span*", "vbz_gpu_match_row*"]
    assert prototype(text, NAMES[1]) == ["vbz_gpu_ctx*", "uint32_t", "const uint32_t*", "const vbz_gpu_sample_ranges*", "uint32_t", "uint32_t*"]
    path, twin = L.vbz_gpu_locate_path_batch.argtypes, L.vbz_gpu_match_path_batch.argtypes
    assert len(path) == len(twin) == 10
    assert [a for a, b in zip(path, twin) if a is not b] == [ctypes.POINTER(_lib.GpuLocate)] and twin[5] is ctypes.POINTER(_lib.GpuMatch)
    assert path[7] is ctypes.POINTER(_lib.GpuMatchPath)
    valid = L.vbz_gpu_query_valid_batch.argtypes
    assert len(valid) == 6 and valid[3] is ctypes.POINTER(_lib.GpuSampleRanges) and valid[1] is ctypes.c_uint32 and valid[4] is ctypes.c_uint32


def test_no_struct_of_their_own():
    """one declaration each of the records the call shares with the match path, at their sizes, in front of the prototype"""
    text = header()
    for name, size, cls in (("vbz_gpu_match_pair", 16, _lib.GpuMatchPair), ("vbz_gpu_match_path", 16, _lib.GpuMatchPath), ("vbz_gpu_match_row", 8, _lib.GpuMatchRow),
                            ("vbz_gpu_match_span", 16, _lib.GpuMatchSpan), ("vbz_gpu_locate", 40, _lib.GpuLocate)):
        assert len(re.findall(r"typedef struct %s\b" % name, text)) == 1, name
        m = re.search(r"\}\s*%s;\s*/\* (\d+) bytes \*/" % name, text)
        assert m and int(m.group(1)) == size == ctypes.sizeof(cls), name
        assert text.index("} %s;" % name) < text.index("vbz_gpu_locate_path_batch("), name
    assert "vbz_gpu_locate_path" not in "".join(re.findall(r"typedef struct (\w+)", text))
    assert [f[0] for f in _lib.GpuMatchPair._fields_] == ["read", "ref", "begin", "end"]


def test_the_header_states_the_rule():
    text = header()
    text = text[text.index("/* Signal locate: the warping path of chosen pairs") : text.index("VBZ_EXPORT int vbz_gpu_query_valid_batch")]
    for phrase in ("path_pair(levels of the read[:n], target[:L], a, b)", "TARGET coordinates", "n = min(valid[read], N)", "c(i, j) = |k_i - g_j|",
                   "row 0 at column a is (c(0, a), a)", "the FIRST of diagonal, up, left", "at j == a:        up",
                   "left while j > a and P[0][j-1].cost == 0", "hit = {cost, end = b, start, rows = n}", "[n_pairs, query_len]",
                   "entries at i >= n are {0, 0}", "begin_0 == start, end_{n-1} == b, begin_i < end_i, begin_{i+1} is end_i - 1 or end_i",
                   "the sum of c over the named cells is cost", "any a' <= start with the", "{0xFFFFFFFF, 0, 0, 0}", "read >= n_reads or ref >= G",
                   "begin >= end, n == 0, L_g == 0 or L_g > target_stride", "end > L_g, or end - begin > max_width", "EVERY entry of hit and rows is written",
                   "16-byte stores", "a multiple of 8 from 8 to 65536", "valid is REQUIRED here", "n_pairs * N * 8, n_reads * N * 4 or G * target_stride beyond 2^46 bytes",
                   "n_pairs == 0 with good arguments returns 0", "min(T', N)", "or 0 for an error verdict", "ranges may be NULL",
                   "query_len outside 8 ... 65536 in multiples of 8",
                   "vbz_gpu_signal_locate_span_batch -> vbz_gpu_query_valid_batch -> vbz_gpu_match_best_batch -> vbz_gpu_locate_path_batch",
                   "nothing at or behind dword", "match_path_pair_words(max_width, query_len)", "No LDS, no barrier, no atomics"):
        assert phrase in text, phrase
    locate = header()
    locate = locate[locate.index("/* Signal locate.") : locate.index("} vbz_gpu_locate;")]
    assert "the path in target coordinates" not in locate and "vbz_gpu_locate_path_batch" in locate


def test_codec_methods():
    p = inspect.signature(batch.GpuCodec.locate_path).parameters
    assert list(p) == ["self", "query", "valid", "target", "target_len", "pairs", "max_width", "locate", "hit", "rows"]
    assert [p[k].default for k in ("locate", "hit", "rows")] == [None, None, None]
    p = inspect.signature(batch.GpuCodec.query_valid).parameters
    assert list(p) == ["self", "result", "query_len", "begin", "end", "out"] and [p[k].default for k in ("begin", "end", "out")] == [None, None, None]


def test_null_context_is_minus_one():
    L = _lib.load()
    m = _lib.GpuLocate()
    path = _lib.GpuMatchPath(8, 0, 0)
    assert L.vbz_gpu_locate_path_batch(None, 0, 0, None, None, ctypes.byref(m), None, ctypes.byref(path), None, None) == -1
    assert L.vbz_gpu_query_valid_batch(None, 0, None, None, 64, None) == -1
