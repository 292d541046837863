"""CPU tests of the pore-model entry points (include/vbz_gpu.h: vbz_gpu_squiggle_batch, vbz_gpu_levels_fit_batch): exported, declared,
listed in _lib.GPU_API, their three structs tied to the header -- sizes 48, 16 and 16, field by field -- the flags' values, the rule stated
in the header, bound by GpuCodec, and refused without a context before anything touches a device."""
import ctypes
import inspect
import re

from test_eventalign_abi import fields
from test_locate_abi import header, prototype
from vbz_compression_amd import _lib, batch

NAMES = ("vbz_gpu_squiggle_batch", "vbz_gpu_levels_fit_batch")


def test_exported_declared_and_listed():
    L = _lib.load()
    text = header()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in _lib.GPU_API, name
        assert getattr(L, name).restype == ctypes.c_int and getattr(L, name).argtypes, name
    assert prototype(text, NAMES[0]) == ["vbz_gpu_ctx*", "const vbz_gpu_squiggle*", "int8_t*", "uint32_t*", "uint32_t*", "float*"]
    assert prototype(text, NAMES[1]) == ["vbz_gpu_ctx*", "uint32_t", "uint32_t", "const vbz_gpu_locate*", "const vbz_gpu_match_pair*",
                                         "const vbz_gpu_match_span*", "const uint32_t*", "const vbz_gpu_level*", "const vbz_gpu_levels_fit*", "const float*",
                                         "vbz_gpu_level_fit*", "float*", "float*", "int64_t*"]
    sq, fit = L.vbz_gpu_squiggle_batch.argtypes, L.vbz_gpu_levels_fit_batch.argtypes
    assert len(sq) == 6 and sq[1] is ctypes.POINTER(_lib.GpuSquiggle)
    assert len(fit) == 14 and fit[1] is ctypes.c_uint32 and fit[2] is ctypes.c_uint32 and fit[3] is ctypes.POINTER(_lib.GpuLocate)
    assert fit[8] is ctypes.POINTER(_lib.GpuLevelsFit)


def test_the_structs_are_the_headers():
    text = header()
    ctype = {"uint32_t": ctypes.c_uint32, "float": ctypes.c_float, "const uint8_t*": ctypes.c_void_p, "const uint32_t*": ctypes.c_void_p,
             "const float*": ctypes.c_void_p}
    for name, size, cls, offsets in (("vbz_gpu_squiggle", 48, _lib.GpuSquiggle, {"k": 0, "n_seqs": 4, "seq_stride": 8, "target_stride": 12, "flags": 16, "quant": 20,
                                                                                 "seq": 24, "seq_len": 32, "model": 40}),
                                     ("vbz_gpu_levels_fit", 16, _lib.GpuLevelsFit, {"max_width": 0, "min_samples": 4, "max_entries": 8, "flags": 12}),
                                     ("vbz_gpu_level_fit", 16, _lib.GpuLevelFit, {"offset": 0, "scale": 4, "used": 8, "ok": 12})):
        assert len(re.findall(r"typedef struct %s\b" % name, text)) == 1, name
        m = re.search(r"\}\s*%s;\s*/\* (\d+) bytes \*/" % name, text)
        assert m and int(m.group(1)) == size == ctypes.sizeof(cls), name
        declared = fields(text, name)
        assert [f for _, f in declared] == [f for f, _ in cls._fields_] == list(offsets), (name, declared)
        for (t, f), (_, ct) in zip(declared, cls._fields_):
            assert ctype[t] is ct and getattr(cls, f).offset == offsets[f], (name, f, t)
        assert text.index("} %s;" % name) < text.index("vbz_gpu_squiggle_batch("), name
    assert re.search(r"#define VBZ_GPU_SQUIGGLE_BOTH\s+1u\b", text) and re.search(r"#define VBZ_GPU_SQUIGGLE_REVERSED\s+2u\b", text)
    assert (_lib.SQUIGGLE_BOTH, _lib.SQUIGGLE_REVERSED) == (1, 2)


def test_the_header_states_the_rule():
    text = header()
    text = text[text.index("/* Pore model on the device") : text.index("VBZ_EXPORT int vbz_gpu_levels_fit_batch")]
    for phrase in ("tests/squiggle_ref.py", "A/a = 0, C/c = 1, G/g = 2, T/t/U/u = 3", "n > seq_stride gives the row or rows", "b'_i = 3 - b_(n-1-i)",
                   "L = n - k + 1 when k <= n, else 0", "L > target_stride also gives 0", "the first\n * base most significant", "L - 1 - j with REVERSED",
                   "strand first, then reversed", "one float32 multiply", "clamp(rint(v), -127, 127)", "+-inf giving +-127", "int8 0 and float +0",
                   "counted in masked[row]", "written whole", "the 32 bits of m", "EVERY entry of all four tables",
                   "rows * target_stride * 4 or S * seq_stride beyond 2^46 bytes", "g = pairs[p].ref", "float64(sum_t) / float64(n_samples_t)",
                   "max(min_samples, 1)", "max_entries != 0", "|m_t| <= 32768 does not hold", "q_t = int64(rint(m_t * 64))", "num = K Sgq - Sg Sq",
                   "|num| < 2^62 and den < 2^47", "none fused", "B = (float64(Sq) - A * float64(Sg)) / float64(K)",
                   "scale = float32(1.0 / (a * float64(quant))) and offset = float32(-b)", "K >= 2, den > 0, num > 0", "offset = -shift",
                   "0 and 1 when the prior is NULL or read >= n_reads", "used = K, or 0 for an\n * invalid pair", "read >= n_reads; ref >= G; W == 0\n * or W > max_width",
                   "end - start != W; L_g == 0 or L_g > target_stride; end > L_g", "EVERY entry of out, offset, scale and sums",
                   "everything vbz_gpu_locate_batch refuses about locate", "n_pairs * max_width * 32 beyond 2^46 bytes",
                   "n_pairs == 0 with good arguments returns 0 and launches nothing", "No LDS, no barrier, no atomics", "tools/time_refit.py"):
        assert phrase in text, phrase


def test_codec_methods():
    p = inspect.signature(batch.GpuCodec.squiggle).parameters
    assert list(p) == ["self", "seq", "seq_len", "model", "k", "target_stride", "quant", "both", "reversed", "level", "target", "target_len", "masked"]
    assert [p[k].default for k in ("quant", "both", "reversed", "level", "target", "target_len", "masked")] == [32.0, False, False, False, None, None, None]
    p = inspect.signature(batch.GpuCodec.levels_fit).parameters
    assert list(p) == ["self", "pairs", "hit", "n_levels", "levels", "target", "target_len", "n_reads", "locate", "min_samples", "max_entries", "prior", "sums",
                       "out", "offset", "scale"]
    assert [p[k].default for k in ("locate", "min_samples", "max_entries", "prior", "sums", "out", "offset", "scale")] == [None, 0, 0, None, False, None, None, None]


def test_null_context_is_minus_one():
    L = _lib.load()
    sq, fit, loc = _lib.GpuSquiggle(), _lib.GpuLevelsFit(8, 0, 0, 0), _lib.GpuLocate()
    assert L.vbz_gpu_squiggle_batch(None, ctypes.byref(sq), None, None, None, None) == -1
    assert L.vbz_gpu_levels_fit_batch(None, 0, 0, ctypes.byref(loc), None, None, None, None, ctypes.byref(fit), None, None, None, None, None) == -1
