"""CPU tests of the signal-trim entry points (include/vbz_gpu.h: vbz_gpu_trim): exported, declared with their struct and macro, listed in
_lib.GPU_API, bound by GpuCodec, and refused without a context before anything touches a device."""
import ctypes
import inspect
import os
import re

from vbz_compression_amd import _lib, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vbz_gpu_signal_trim_batch", "vbz_gpu_pod5_signal_trim_batch")


def header():
    return open(os.path.join(ROOT, "include", "vbz_gpu.h")).read()


def test_exported_declared_and_listed():
    L = _lib.load()
    text = header()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in _lib.GPU_API, name
        assert re.search(r"VBZ_EXPORT\s+int\s+" + name + r"\s*\(", text), name
        assert getattr(L, name).restype == ctypes.c_int and len(getattr(L, name).argtypes) == 10, name


def test_struct_layout():
    text = header()
    S = _lib.GpuTrim
    assert ctypes.sizeof(S) == 32
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("window", 0), ("min_elements", 4), ("min_trim", 8), ("max_samples", 12),
                                                                   ("threshold_factor", 16), ("max_fraction", 20), ("flags", 24), ("reserved", 28)]
    fields = re.search(r"typedef struct vbz_gpu_trim\s*\{(.*?)\}\s*vbz_gpu_trim;", text, re.S).group(1)
    decl = re.findall(r"^\s*(uint32_t|float)\s+(\w+);", fields, re.M)
    assert [n for _, n in decl] == [f[0] for f in S._fields_]
    assert [t for t, _ in decl] == ["uint32_t"] * 4 + ["float"] * 2 + ["uint32_t"] * 2
    assert [f[1] for f in S._fields_] == [ctypes.c_uint32] * 4 + [ctypes.c_float] * 2 + [ctypes.c_uint32] * 2


def test_macro():
    m = re.search(r"#define\s+VBZ_GPU_TRIM_REJECT_AT_END\s+(\w+)", header())
    assert m and int(m.group(1).rstrip("uU"), 0) == _lib.VBZ_GPU_TRIM_REJECT_AT_END == 1


def test_trim_dataclass():
    t = batch.Trim().c_struct()
    assert (t.window, t.min_elements, t.min_trim, t.max_samples, t.flags, t.reserved) == (40, 3, 10, 8000, 0, 0)
    assert abs(t.threshold_factor - 2.4) < 1e-6 and t.max_fraction == 1.0
    t = batch.Trim(window=64, min_elements=0, min_trim=0, max_samples=100, threshold_factor=-1.5, max_fraction=0.3, reject_at_end=True).c_struct()
    assert (t.window, t.min_elements, t.min_trim, t.max_samples, t.flags) == (64, 0, 0, 100, _lib.VBZ_GPU_TRIM_REJECT_AT_END)
    assert t.threshold_factor == -1.5 and abs(t.max_fraction - 0.3) < 1e-6


def test_codec_methods():
    for name in ("signal_trim", "pod5_signal_trim"):
        p = inspect.signature(getattr(batch.GpuCodec, name)).parameters
        assert {"norm", "trim", "out", "shift_scale", "signed", "begin", "end", "stats"} <= set(p), name
    assert "sized" in inspect.signature(batch.GpuCodec.signal_trim).parameters


def test_null_context_or_batch_is_minus_one():
    L = _lib.load()
    b = _lib.GpuBatch()
    opts = _lib.CompressionOptions(True, 2, 1, 1)
    popts = batch.pod5_options()
    m = batch.MED_MAD.c_struct()
    r = _lib.GpuPod5Reads()
    g = _lib.GpuSampleRanges()
    t = batch.Trim().c_struct()
    for ctx_b in ((None, ctypes.byref(b)), (None, None)):
        assert L.vbz_gpu_signal_trim_batch(*ctx_b, ctypes.byref(opts), 0, 1, ctypes.byref(m), ctypes.byref(g), ctypes.byref(t), None, None) == -1
        assert L.vbz_gpu_signal_trim_batch(*ctx_b, ctypes.byref(opts), 0, 1, ctypes.byref(m), None, None, None, None) == -1
        assert L.vbz_gpu_pod5_signal_trim_batch(*ctx_b, ctypes.byref(popts), 1, ctypes.byref(r), ctypes.byref(m), ctypes.byref(g), ctypes.byref(t), None,
                                                None) == -1
