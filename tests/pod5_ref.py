"""numpy statement of POD5's signal codec (include/vbz_gpu.h: VBZ_GPU_VERSION_POD5), written from the published format: svb16 of the
zig-zag deltas of a row's int16 samples, then one zstd frame.  A row as pod5 writes it is zstd_compress(svb16_encode(x), level 1) through
oracle_lib's libzstd -- the bytes pod5's compress_signal writes with that libzstd."""
import json
import os

import numpy as np

import oracle_lib as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROW = 102400   # samples per signal row of the golden reads (pod5 cuts reads into rows of this size)


def key_len(n):
    return (n + 7) // 8


def svb16_max(n):
    return key_len(n) + 2 * n


def zstd_bound(n):   # ZSTD_COMPRESSBOUND
    return n + (n >> 8) + (((128 << 10) - n) >> 11 if n < (128 << 10) else 0)


def max_compressed_size(n):
    return zstd_bound(svb16_max(n))


def zigzag(x):
    """the zig-zag deltas z_j (uint16) of the int16 samples x (delta from 0 at the row's start, wrap-around)"""
    u = np.asarray(x).astype(np.int16).view(np.uint16).astype(np.uint32)
    d = (u - np.concatenate([[0], u[:-1]]).astype(np.uint32)) & 0xFFFF
    s = (d >> 15) * 0xFFFF   # int16(d) >> 15, as 16 bits
    return (((d << 1) ^ s) & 0xFFFF).astype(np.uint16)


def svb16_encode(x):
    """the svb16 stream of int16 samples x (numpy uint8)"""
    z = zigzag(x).astype(np.uint32)
    n = len(z)
    two = z > 0xFF
    keys = np.packbits(np.concatenate([two, np.zeros(key_len(n) * 8 - n, bool)]), bitorder="little") if n else np.zeros(0, np.uint8)
    lo = (z & 0xFF).astype(np.uint8)
    hi = (z >> 8).astype(np.uint8)
    data = np.stack([lo, hi], 1).reshape(-1)[np.stack([np.ones(n, bool), two], 1).reshape(-1)]
    return np.concatenate([keys, data]).astype(np.uint8)


def svb16_decode(stream, n):
    """int16 samples of a stream that holds n; None when its length is not K + n + popcount(the first n key bits)"""
    s = np.asarray(stream, np.uint8)
    K = key_len(n)
    if len(s) < K:
        return None
    two = np.unpackbits(s[:K], bitorder="little")[:n].astype(bool)
    if len(s) != K + n + int(two.sum()):
        return None
    width = 1 + two.astype(np.int64)
    start = K + np.concatenate([[0], np.cumsum(width)[:-1]]).astype(np.int64) if n else np.zeros(0, np.int64)
    z = s[start].astype(np.uint32)
    z[two] |= s[start[two] + 1].astype(np.uint32) << 8
    d = (z >> 1) ^ ((0 - (z & 1)) & 0xFFFF)
    return (np.cumsum(d.astype(np.uint64)) & 0xFFFF).astype(np.uint16).view(np.int16)


def compress_row(x, level=1):
    """a row as pod5 writes it: one libzstd frame of the svb16 stream"""
    return O.zstd_compress(svb16_encode(x), level)


def decompress_row(frame, n):
    """int16 samples of a row, None for any failure (libzstd's, or the stream's length)"""
    s = O.zstd_decompress(frame, svb16_max(n))
    return None if s is None else svb16_decode(s, n)


def golden_reads():
    """the real signal of tests/golden: the reads of fast5_chunks (sized v0 chunks decoded by the reference), and test_data_read.i16"""
    idx = json.load(open(os.path.join(GOLDEN, "fast5_chunks.json")))
    blob = np.fromfile(os.path.join(GOLDEN, "fast5_chunks.bin"), np.uint8)
    reads = []
    for e in idx:
        raw = O.decompress(blob[e["chunk_offset"] : e["chunk_offset"] + e["chunk_size"]], 2 * e["samples"], O.options(True, 2, 1, 0), sized=True)
        reads.append(raw.view(np.int16))
    reads.append(np.fromfile(os.path.join(GOLDEN, "test_data_read.i16"), np.int16))
    return reads


def golden_rows():
    """the golden reads cut into rows of ROW samples: (rows, the read of each row)"""
    rows, owner = [], []
    for k, x in enumerate(golden_reads()):
        for s in range(0, len(x), ROW):
            rows.append(x[s : s + ROW].copy())
            owner.append(k)
    return rows, owner
