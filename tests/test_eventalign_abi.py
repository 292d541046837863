"""CPU tests of the event-space alignment entry points (include/vbz_gpu.h: vbz_gpu_events_query_batch, vbz_gpu_locate_levels_batch):
exported, declared, listed in _lib.GPU_API, the two structs of their own and the event table they share tied to the header -- sizes 16, 32
and 32, field by field -- the rule stated in the header, bound by GpuCodec, and refused without a context before anything touches a device."""
import ctypes
import inspect
import re

from test_locate_abi import header, prototype
from vbz_compression_amd import _lib, batch

NAMES = ("vbz_gpu_events_query_batch", "vbz_gpu_locate_levels_batch")


def test_exported_declared_and_listed():
    L = _lib.load()
    text = header()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in _lib.GPU_API, name
        assert getattr(L, name).restype == ctypes.c_int and getattr(L, name).argtypes, name
    assert prototype(text, NAMES[0]) == ["vbz_gpu_ctx*", "uint32_t", "const uint32_t*", "const vbz_gpu_events*", "const vbz_gpu_event*",
                                         "const vbz_gpu_events_query*", "float*", "uint32_t*", "uint32_t*"]
    assert prototype(text, NAMES[1]) == ["vbz_gpu_ctx*", "uint32_t", "uint32_t", "uint32_t", "uint32_t", "const vbz_gpu_match_pair*", "const vbz_gpu_match_span*",
                                         "const vbz_gpu_match_row*", "const uint32_t*", "const vbz_gpu_events*", "const vbz_gpu_event*",
                                         "const vbz_gpu_event_moments*", "uint32_t*", "vbz_gpu_level*"]
    q, lv = L.vbz_gpu_events_query_batch.argtypes, L.vbz_gpu_locate_levels_batch.argtypes
    assert len(q) == 9 and q[1] is ctypes.c_uint32 and q[3] is ctypes.POINTER(_lib.GpuEvents) and q[5] is ctypes.POINTER(_lib.GpuEventsQuery)
    assert len(lv) == 14 and all(a is ctypes.c_uint32 for a in lv[1:5]) and lv[9] is ctypes.POINTER(_lib.GpuEvents)


def fields(text, name):
    body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (name, name), text, re.S).group(1)
    return [(m.group(1).strip(), m.group(2)) for m in re.finditer(r"^\s*((?:const\s+)?\w+\*?)\s+(\w+);", body, re.M)]


def test_the_structs_are_the_headers():
    text = header()
    ctype = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int64_t": ctypes.c_int64, "const uint64_t*": ctypes.c_void_p,
             "const uint32_t*": ctypes.c_void_p}
    for name, size, cls, offsets in (("vbz_gpu_events_query", 16, _lib.GpuEventsQuery, {"query_len": 0, "min_n": 4, "flags": 8, "reserved": 12}),
                                     ("vbz_gpu_level", 32, _lib.GpuLevel, {"first_sample": 0, "end_sample": 4, "n_samples": 8, "n_entries": 12, "sum": 16,
                                                                            "sumsq": 24}),
                                     ("vbz_gpu_events", 32, _lib.GpuEvents, {"event_rows": 0, "event_first": 8, "start": 16, "flags": 24, "reserved": 28})):
        assert len(re.findall(r"typedef struct %s\b" % name, text)) == 1, name
        m = re.search(r"\}\s*%s;\s*/\* (\d+) bytes \*/" % name, text)
        assert m and int(m.group(1)) == size == ctypes.sizeof(cls), name
        declared = fields(text, name)
        assert [f for _, f in declared] == [f for f, _ in cls._fields_] == list(offsets), (name, declared)
        for (t, f), (_, ct) in zip(declared, cls._fields_):
            assert ctype[t] is ct and getattr(cls, f).offset == offsets[f], (name, f, t)
        assert text.index("} %s;" % name) < text.index("vbz_gpu_locate_levels_batch("), name


def test_the_header_states_the_rule():
    text = header()
    text = text[text.index("/* Event-space alignment.") : text.index("VBZ_EXPORT int vbz_gpu_locate_levels_batch")]
    for phrase in ("segment -> events -> events_query -> locate_span -> match_best -> locate_path -> locate_levels", "tests/eventalign_ref.py",
                   "records[c].n >= min_n", "the 32 bits copied", "index[i][k] = c - c0", "valid[i] is the number kept, at most N", "index may be NULL",
                   "result may be\n * NULL", "vbz_gpu_query_valid_batch", "event_first[i] > event_first[i + 1], event_first[i + 1] > event_rows",
                   "more than 2^31 - 1 rows", "events->start is not read", "EVERY entry of query, valid and index is written",
                   "n_reads * N * 4 or event_rows * 16 beyond 2^46 bytes", "[n_pairs, max_width]", "E_j = {k < n : begin_k <= j < end_k}",
                   "c_k = event_first[read] + index[read][k]", "modulo 2^32 and 2^64", "differences of prefix sums", "counts in each",
                   "n_levels[p] = end - start", "32 zero bytes", "read >= n_reads", "n > query_len", "begin_0 == start, end_(n-1) == end, begin_k < end_k",
                   "one of end_k - 1 and\n * end_k", "EVERY entry of n_levels and levels", "16-byte stores", "start REQUIRED here",
                   "8 ... 65536 in multiples\n * of 8", "no LDS, no barrier, no atomics", "O(n + width) a pair", "tools/time_eventalign.py"):
        assert phrase in text, phrase


def test_codec_methods():
    p = inspect.signature(batch.GpuCodec.events_query).parameters
    assert list(p) == ["self", "event_first", "records", "query_len", "min_n", "result", "index", "query", "valid"]
    assert [p[k].default for k in ("min_n", "result", "index", "query", "valid")] == [0, None, True, None, None]
    p = inspect.signature(batch.GpuCodec.locate_levels).parameters
    assert list(p) == ["self", "pairs", "hit", "rows", "event_first", "start", "records", "moments", "max_width", "index", "n_levels", "levels"]
    assert [p[k].default for k in ("index", "n_levels", "levels")] == [None, None, None]


def test_null_context_is_minus_one():
    L = _lib.load()
    ev, q = _lib.GpuEvents(), _lib.GpuEventsQuery(8, 0, 0, 0)
    assert L.vbz_gpu_events_query_batch(None, 0, None, ctypes.byref(ev), None, ctypes.byref(q), None, None, None) == -1
    assert L.vbz_gpu_locate_levels_batch(None, 0, 0, 8, 8, None, None, None, None, ctypes.byref(ev), None, None, None, None) == -1
