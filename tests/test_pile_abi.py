"""CPU tests of the pile-up entry points (include/vbz_gpu_pile.h): exported, declared in that header and listed in _lib.PILE_API -- a list of
its own, disjoint from GPU_API, because C_API + GPU_API are held to a recorded table no change edits -- their three structs tied to the header
field by field, the flags' values, the ctypes prototypes held to tests/golden/prototypes_pile.json (this module's own output, `python
tests/test_pile_abi.py`), argument counts equal to the header's, bound by GpuCodec, and refused without a context before anything touches a
device."""
import ctypes
import inspect
import json
import os
import re

from test_eventalign_abi import fields
from test_locate_abi import prototype
from test_prototypes_abi import spell
from vbz_compression_amd import _lib, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "prototypes_pile.json")
NAMES = ("vbz_gpu_levels_pile_batch", "vbz_gpu_squiggle_kmers_batch", "vbz_gpu_pile_kmers_batch", "vbz_gpu_model_update_batch")


def header():
    return open(os.path.join(ROOT, "include", "vbz_gpu_pile.h")).read()


def declared(L):
    return {name: [spell(getattr(L, name).restype), [spell(a) for a in getattr(L, name).argtypes]] for name in _lib.PILE_API}


def test_exported_declared_and_listed():
    L = _lib.load()
    text = header()
    assert tuple(_lib.PILE_API) == NAMES == tuple(_lib.PILE_PROTOTYPES)
    assert re.findall(r"VBZ_EXPORT\s+int\s+(\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)) == list(NAMES)
    assert '#include "vbz_gpu.h"' in text
    for name in NAMES:
        assert hasattr(L, name), name
        assert getattr(L, name).restype == ctypes.c_int and len(getattr(L, name).argtypes) == len(prototype(text, name)), name
    assert prototype(text, NAMES[0]) == ["vbz_gpu_ctx*", "uint32_t", "uint32_t", "const vbz_gpu_locate*", "const vbz_gpu_match_pair*", "const vbz_gpu_match_span*",
                                         "const uint32_t*", "const vbz_gpu_level*", "const vbz_gpu_levels_pile*", "const vbz_gpu_level_fit*", "uint64_t*"]
    assert prototype(text, NAMES[1]) == ["vbz_gpu_ctx*", "const vbz_gpu_squiggle*", "uint32_t*", "uint32_t*"]
    assert prototype(text, NAMES[2]) == ["vbz_gpu_ctx*", "const vbz_gpu_pile_kmers*", "const uint32_t*", "const uint32_t*", "const uint64_t*", "uint64_t*"]
    assert prototype(text, NAMES[3]) == ["vbz_gpu_ctx*", "const vbz_gpu_model_update*", "const uint64_t*", "const float*", "float*", "float*"]
    P = ctypes.POINTER
    assert L.vbz_gpu_levels_pile_batch.argtypes[3] is P(_lib.GpuLocate) and L.vbz_gpu_levels_pile_batch.argtypes[8] is P(_lib.GpuLevelsPile)
    assert L.vbz_gpu_squiggle_kmers_batch.argtypes[1] is P(_lib.GpuSquiggle) and L.vbz_gpu_pile_kmers_batch.argtypes[1] is P(_lib.GpuPileKmers)
    assert L.vbz_gpu_model_update_batch.argtypes[1] is P(_lib.GpuModelUpdate)


def test_the_names_stand_apart_from_the_recorded_lists():
    assert not set(NAMES) & set(_lib.C_API + _lib.GPU_API) and not set(NAMES) & set(_lib.PROTOTYPES)
    main = open(os.path.join(ROOT, "include", "vbz_gpu.h")).read()
    assert not any(name in main for name in NAMES)


def test_the_recorded_prototypes_are_held():
    want = json.load(open(GOLDEN))
    got = declared(_lib.load())
    assert sorted(want) == sorted(NAMES)
    for name in NAMES:
        assert got[name] == want[name], (name, got[name], want[name])


def test_the_structs_are_the_headers():
    text = header()
    ctype = {"uint32_t": ctypes.c_uint32, "float": ctypes.c_float}
    for name, size, cls, offsets in (("vbz_gpu_levels_pile", 32, _lib.GpuLevelsPile, {"max_width": 0, "min_samples": 4, "max_entries": 8, "flags": 12, "fix": 16,
                                                                                     "reserved0": 20, "reserved1": 24, "reserved2": 28}),
                                     ("vbz_gpu_pile_kmers", 16, _lib.GpuPileKmers, {"k": 0, "rows": 4, "target_stride": 8, "flags": 12}),
                                     ("vbz_gpu_model_update", 16, _lib.GpuModelUpdate, {"k": 0, "min_obs": 4, "flags": 8, "fix": 12})):
        assert len(re.findall(r"typedef struct %s\b" % name, text)) == 1, name
        m = re.search(r"\}\s*%s;\s*/\* (\d+) bytes \*/" % name, text)
        assert m and int(m.group(1)) == size == ctypes.sizeof(cls), name
        declared_fields = fields(text, name)
        assert [f for _, f in declared_fields] == [f for f, _ in cls._fields_] == list(offsets), (name, declared_fields)
        for (t, f), (_, ct) in zip(declared_fields, cls._fields_):
            assert ctype[t] is ct and getattr(cls, f).offset == offsets[f], (name, f, t)
    for macro, value, mine in (("CLEAR", 1, _lib.PILE_CLEAR), ("REQUIRE_OK", 2, _lib.PILE_REQUIRE_OK), ("DIRECT", 4, _lib.PILE_DIRECT)):
        assert re.search(r"#define VBZ_GPU_PILE_%s\s+%du\b" % (macro, value), text) and mine == value, macro
    assert _lib.KMER_MARK == 0xFFFFFFFF and "0xFFFFFFFF" in text


def test_the_header_states_the_rule():
    text = header()
    text = text[: text.index("#ifndef VBZ_GPU_PILE_H")]
    for phrase in ("tests/pile_ref.py", "pile[q * n_cells + c]", "n + 2^32 * skipped", "modulo 2^64", "g *\n * target_stride + j", "n_cells = 4^k",
                   "512-byte atomic instruction", "exactly that call's test", "0 and 1 when fit is NULL", "fit[p].ok == 0 contributes nothing", "none fused",
                   "m = float64(sum) / float64(n_samples)", "v = (m + float64(o)) * float64(s)", "w = v * float64(fix)", "max(min_samples, 1)",
                   "max_entries != 0", "|w| <= 2^24\n * does not hold (NaN included)", "u = int64(rint(w))", "sumsq cannot wrap below 2^15 observations",
                   "carries into the high half at 2^32 observations", "reproducible bit for bit", "zeroed on the context's stream before the adds",
                   "Nothing outside cells [g][start, end) of contributing pairs", "G * target_stride * 32 beyond 2^46 bytes", "with CLEAR it clears",
                   "squiggle->model is not read and may be NULL", "at and behind L", "no address is formed from it", "all zero are skipped",
                   "low 32 bits of the count word", "n >= max(min_obs, 1)", "float32(mean / float64(fix))", "sqrt(max(var, 0))", "the 32 bits of prior[i]",
                   "same pointer as model", "No LDS, no scratch, no barrier", "tools/time_pile.py", "profiles/pile_time.json"):
        assert phrase in text, phrase


def test_codec_methods():
    p = inspect.signature(batch.GpuCodec.squiggle_kmers).parameters
    assert list(p) == ["self", "seq", "seq_len", "k", "target_stride", "both", "reversed", "kmer", "target_len"]
    p = inspect.signature(batch.GpuCodec.levels_pile).parameters
    assert list(p) == ["self", "pairs", "hit", "n_levels", "levels", "target", "target_len", "n_reads", "fix", "fit", "require_ok", "clear", "locate", "min_samples",
                       "max_entries", "pile"]
    assert [p[k].default for k in ("fix", "fit", "require_ok", "clear", "locate", "min_samples", "max_entries", "pile")] == [256.0, None, False, False, None, 0, 0, None]
    p = inspect.signature(batch.GpuCodec.pile_kmers).parameters
    assert list(p) == ["self", "pile", "kmer", "target_len", "k", "clear", "direct", "kmer_pile"]
    p = inspect.signature(batch.GpuCodec.model_update).parameters
    assert list(p) == ["self", "kmer_pile", "prior", "k", "fix", "min_obs", "sd", "model"]
    assert [p[k].default for k in ("fix", "min_obs", "sd", "model")] == [256.0, 0, False, None]


def test_null_context_is_minus_one():
    L = _lib.load()
    loc, par, sq = _lib.GpuLocate(), _lib.GpuLevelsPile(8, 0, 0, 0, 256.0, 0, 0, 0), _lib.GpuSquiggle()
    assert L.vbz_gpu_levels_pile_batch(None, 0, 0, ctypes.byref(loc), None, None, None, None, ctypes.byref(par), None, None) == -1
    assert L.vbz_gpu_squiggle_kmers_batch(None, ctypes.byref(sq), None, None) == -1
    assert L.vbz_gpu_pile_kmers_batch(None, ctypes.byref(_lib.GpuPileKmers(3, 1, 16, 0)), None, None, None, None) == -1
    assert L.vbz_gpu_model_update_batch(None, ctypes.byref(_lib.GpuModelUpdate(3, 0, 0, 256.0)), None, None, None, None) == -1


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump(declared(_lib.load()), f, indent=0, sort_keys=True)
        f.write("\n")
