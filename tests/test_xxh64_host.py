"""CPU tests of vbz_compression_amd/csrc/xxh64.h, the serial XXH64 (seed 0) behind the zstd content checksum: built with g++ and
compared with libzstd's own ZSTD_XXH64 (libzstd.so.1, the library tests/oracle_lib.py loads)."""
import ctypes
import ctypes.util
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "xxh64_harness.cpp")
CSRC = os.path.join(ROOT, "vbz_compression_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("xxh64") / "libxxh64_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-I" + CSRC, "-o", so, SRC])
    L = ctypes.CDLL(so)
    L.h_xxh64.restype = ctypes.c_uint64
    L.h_xxh64.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    return L


@pytest.fixture(scope="module")
def libzstd():
    name = ctypes.util.find_library("zstd") or "libzstd.so.1"
    try:
        L = ctypes.CDLL(name)
    except OSError:
        L = ctypes.CDLL("libzstd.so.1")
    L.ZSTD_XXH64.restype = ctypes.c_uint64
    L.ZSTD_XXH64.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64]
    return L


def _ptr(a, off=0):
    return a.ctypes.data + off


def test_known_values(harness):
    # published XXH64 (seed 0) values: the empty input and "abc"
    e = np.zeros(1, np.uint8)
    assert harness.h_xxh64(_ptr(e), 0) == 0xEF46DB3751D8E999
    abc = np.frombuffer(b"abc", np.uint8).copy()
    assert harness.h_xxh64(_ptr(abc), 3) == 0x44BC2CF5AD770999


def test_every_length_to_300_unaligned(harness, libzstd):
    rng = np.random.default_rng(11)
    buf = rng.integers(0, 256, 300 + 16, dtype=np.uint8)
    for start in (0, 1, 3, 5, 7, 8, 13):
        for n in range(0, 301):
            if start + n > buf.nbytes:
                continue
            assert harness.h_xxh64(_ptr(buf, start), n) == libzstd.ZSTD_XXH64(_ptr(buf, start), n, 0), (start, n)


def test_one_mebibyte(harness, libzstd):
    rng = np.random.default_rng(12)
    buf = rng.integers(0, 256, (1 << 20) + 8, dtype=np.uint8)
    for start, n in ((0, 1 << 20), (3, (1 << 20) + 5), (1, (1 << 20) - 29)):
        assert harness.h_xxh64(_ptr(buf, start), n) == libzstd.ZSTD_XXH64(_ptr(buf, start), n, 0)
