"""CPU tests of the POD5 codec's ABI (include/vbz_gpu.h: VBZ_GPU_VERSION_POD5, vbz_gpu_pod5_max_compressed_size): exported and declared,
the bound against its formula, NULL contexts refused, and the single-buffer API of vbz.h refusing the version before it touches a device."""
import ctypes
import os
import re

import numpy as np

import pod5_ref as P
from vbz_compression_amd import _lib, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "vbz_gpu_pod5_max_compressed_size"
POD5 = 0x35444F50


def test_exported_and_declared():
    L = _lib.load()
    text = open(os.path.join(ROOT, "include", "vbz_gpu.h")).read()
    assert hasattr(L, NAME) and NAME in _lib.GPU_API
    assert re.search(r"VBZ_EXPORT\s+uint64_t\s+" + NAME + r"\s*\(\s*uint32_t\s+\w+\s*\)", text)
    assert re.search(r"#define\s+VBZ_GPU_VERSION_POD5\s+0x35444F50u", text)
    assert _lib.VBZ_GPU_VERSION_POD5 == POD5 == int.from_bytes(b"POD5", "little")
    o = batch.pod5_options()
    assert (o.perform_delta_zig_zag, o.integer_size, o.zstd_compression_level, o.vbz_version) == (True, 2, 1, POD5)
    assert batch.pod5_options(3).zstd_compression_level == 3


def test_bound_formula():
    L = _lib.load()
    for n in [0, 1, 7, 8, 9, 1000, 58253, 58254, 100000, 102400, 1 << 20, 20_000_000, 2**31 - 1, 2**32 - 1]:
        k = (n + 7) // 8
        svb = k + 2 * n
        want = svb + (svb >> 8) + (((128 << 10) - svb) >> 11 if svb < (128 << 10) else 0)
        assert L.vbz_gpu_pod5_max_compressed_size(n) == want == P.max_compressed_size(n), n
        assert batch.pod5_max_compressed_size(n) == want


def test_null_context_is_minus_one():
    L = _lib.load()
    b = _lib.GpuBatch()
    o = batch.pod5_options()
    assert L.vbz_gpu_compress_batch(None, ctypes.byref(b), ctypes.byref(o), 0) == -1
    assert L.vbz_gpu_decompress_batch(None, ctypes.byref(b), ctypes.byref(o), 0) == -1
    assert L.vbz_gpu_svb_compress_batch(None, ctypes.byref(b), 2, 1, POD5) == -1
    assert L.vbz_gpu_svb_decompress_batch(None, ctypes.byref(b), 2, 1, POD5) == -1


def test_single_buffer_api_refuses_the_version():
    L = _lib.load()
    x = np.arange(1000, dtype=np.int16)
    out = np.zeros(8192, np.uint8)
    for level in (0, 1):
        o = _lib.CompressionOptions(True, 2, level, POD5)
        assert L.vbz_max_compressed_size(x.nbytes, ctypes.byref(o)) == _lib.VBZ_VERSION_ERROR
        assert L.vbz_compress(x.ctypes.data, x.nbytes, out.ctypes.data, out.nbytes, ctypes.byref(o)) == _lib.VBZ_VERSION_ERROR
        assert L.vbz_decompress(out.ctypes.data, 64, x.ctypes.data, x.nbytes, ctypes.byref(o)) == _lib.VBZ_VERSION_ERROR


def test_read_layout():
    rows = [3, 5, 2, 7, 1, 0, 4]
    lay = batch.pod5_read_layout(rows, [0, 3, 3, 6])
    assert lay.read_len.tolist() == [10, 0, 8, 4]
    assert lay.read_off.tolist() == [0, 32, 32, 48] and lay.total == 64
    assert lay.dst_off.tolist() == [0, 6, 16, 32, 46, 48, 48]
    assert lay.dst_cap.tolist() == [6, 10, 4, 14, 2, 0, 8]
    lay4 = batch.pod5_read_layout(rows, [0, 3, 3, 6], elem=4, align=64)
    assert lay4.read_off.tolist() == [0, 64, 64, 128] and lay4.dst_off.tolist() == [0, 12, 32, 64, 92, 96, 128]
