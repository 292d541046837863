"""Host harness around vbz_compression_amd/csrc/zstd_entropy.h, zstd_tables.h and zstd_frame.h (tests only): the
serial statements of the Huffman table construction and of the decoders' table and header readers, compiled with
g++, driven through ctypes."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "entropy_harness.cpp")
HDR = os.path.join(ROOT, "vbz_compression_amd", "csrc", "zstd_entropy.h")
TABLES = os.path.join(ROOT, "vbz_compression_amd", "csrc", "zstd_tables.h")
FRAME = os.path.join(ROOT, "vbz_compression_amd", "csrc", "zstd_frame.h")
SO = os.path.join(HERE, "host", "libentropy_harness.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO) or max(os.path.getmtime(f) for f in (SRC, HDR, TABLES, FRAME)) > os.path.getmtime(SO):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.dirname(HDR), "-o", SO, SRC])
        _lib = ctypes.CDLL(SO)
    return _lib


def tree_description(data, package_merge=False):
    """(table log, code lengths[256], tree description bytes) for the byte histogram of `data`,
    as libzstd's HUF_buildCTable / HUF_writeCTable produce them for a block of len(data) <= 128 KiB;
    package_merge: code lengths by huf_build_pm (what the device encoder builds) instead of libzstd's construction."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    return tree_description_counts(np.bincount(data, minlength=256), package_merge)


def tree_description_counts(counts, package_merge=False):
    """tree_description for a region with the byte histogram counts[256] (at least two values occur)"""
    H = lib()
    cnt = np.ascontiguousarray(counts, dtype=np.uint32)
    maxsym = int(np.nonzero(cnt)[0].max())
    u8p, u16p, u32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_uint32)
    n = min(int(cnt.sum()), 128 << 10)
    hl = H.h_optimal_table_log(11, n, maxsym, 1)
    nb = np.zeros(256, np.uint8)
    code = np.zeros(256, np.uint16)
    tl = (H.h_huf_build_pm if package_merge else H.h_huf_build)(cnt.ctypes.data_as(u32p), maxsym, hl, nb.ctypes.data_as(u8p), code.ctypes.data_as(u16p))
    out = np.zeros(300, np.uint8)
    ts = H.h_huf_write_tree(out.ctypes.data_as(u8p), 300, nb.ctypes.data_as(u8p), maxsym, tl)
    return tl, nb, (bytes(out[:ts]) if ts > 0 else None)


def fse_read_ncount(desc, max_symbol, max_log):
    """zstd_tables.h's FSE table description reader over the bytes `desc`: (bytes used or -1, log, normalised counts)."""
    desc = np.frombuffer(bytes(desc), np.uint8).copy()
    norm = np.zeros(256, np.int16)
    log, nsym = ctypes.c_int(0), ctypes.c_int(0)
    r = lib().h_fse_read_ncount(desc.ctypes.data_as(ctypes.c_void_p), len(desc), max_symbol, max_log, norm.ctypes.data_as(ctypes.c_void_p),
                                ctypes.byref(log), ctypes.byref(nsym))
    return (r, log.value, norm[: nsym.value].copy()) if r >= 0 else (r, None, None)


def fse_build(norm, log):
    """zstd_tables.h's FSE decoding table: None, or the cells (symbol | nbBits << 8 | base << 16)."""
    norm = np.ascontiguousarray(norm, np.int16)
    cells = np.zeros(1 << log, np.uint32)
    r = lib().h_fse_build(norm.ctypes.data_as(ctypes.c_void_p), len(norm), log, cells.ctypes.data_as(ctypes.c_void_p))
    return cells if r == 0 else None


def huf_read_weights(desc, max_log):
    """zstd_tables.h's tree description reader: (bytes used, -1 or -2; table log; weights, the implied last one included)."""
    desc = np.frombuffer(bytes(desc), np.uint8).copy()
    w = np.zeros(256, np.uint8)
    nw, log = ctypes.c_int(0), ctypes.c_int(0)
    r = lib().h_huf_read_weights(desc.ctypes.data_as(ctypes.c_void_p), len(desc), max_log, w.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nw),
                                 ctypes.byref(log))
    return (r, log.value, w[: nw.value].copy()) if r >= 0 else (r, None, None)


def parse_first_block_literals(frame):
    """For a zstd frame: (literals type, regenerated size, compressed size, tree description bytes or None,
    number-of-sequences byte) of its first block, or None if that block is not a compressed block."""
    b = bytes(frame)
    fhd = b[4]
    single = (fhd >> 5) & 1
    pos = 5 + (0 if single else 1) + [1 if single else 0, 2, 4, 8][fhd >> 6]
    bh = b[pos] | b[pos + 1] << 8 | b[pos + 2] << 16
    pos += 3
    if (bh >> 1) & 3 != 2:
        return None
    v = int.from_bytes(b[pos : pos + 5], "little")
    t, fmt = v & 3, (v >> 2) & 3
    if t < 2:
        return (t, None, None, None, None)
    if fmt < 2:
        regen, cs, h = (v >> 4) & 0x3FF, (v >> 14) & 0x3FF, 3
    elif fmt == 2:
        regen, cs, h = (v >> 4) & 0x3FFF, (v >> 18) & 0x3FFF, 4
    else:
        regen, cs, h = (v >> 4) & 0x3FFFF, (v >> 22) & 0x3FFFF, 5
    q = pos + h
    tree = None
    if t == 2:
        hb = b[q]
        tl = 1 + hb if hb < 128 else 1 + (hb - 127 + 1) // 2
        tree = b[q : q + tl]
    return (t, regen, cs, tree, b[q + cs])


def weights_report(nb, maxsym, tl):
    """The way huf_write_tree takes for the code lengths nb[0 .. maxsym] at table log tl: (method, kind, low, size) --
    method 0: the weights are never normalised (all equal, every value once, fewer than two), 1 / 2: fse_normalize's first / second
    method; kind 'fse', 'direct' or 'none' (no description can be written); low: weight values given the low-probability count;
    size: bytes of the description."""
    w = np.array([tl + 1 - int(x) if x else 0 for x in nb[:maxsym]], np.uint8)
    out = np.zeros(4, np.uint32)
    r = lib().h_weights_report(w.ctypes.data_as(ctypes.c_void_p), len(w), out.ctypes.data_as(ctypes.c_void_p))
    assert r == 0, "the restated choice between the normalisation methods disagrees with fse_normalize"
    return int(out[0]), ("fse", "direct", "none")[int(out[1])], int(out[2]), int(out[3])


def frame_trailers(frame):
    """The library's skippable frames behind a zstd frame: {magic: payload bytes}."""
    b = bytes(frame)
    out = {}
    pos = [end for _, _, end in walk_blocks(b)][-1] + (4 if (b[4] >> 2) & 1 else 0)
    while pos + 8 <= len(b):
        magic, size = int.from_bytes(b[pos : pos + 4], "little"), int.from_bytes(b[pos + 4 : pos + 8], "little")
        if magic & 0xFFFFFFF0 != 0x184D2A50 or pos + 8 + size > len(b):
            break
        out[magic] = b[pos + 8 : pos + 8 + size]
        pos += 8 + size
    return out


def walk_blocks(frame):
    """Every block of a zstd frame with a content size, in order: (block type, literals, end offset of the block) -- block type 0 raw,
    1 RLE (literals None; see `size` below), 2 compressed with literals = parse_first_block_literals' tuple (literals type, regenerated
    size, compressed size, tree description or None, number of sequences -- the whole count, not its first byte).  For raw and RLE
    blocks `literals` is (None, block size, None, None, 0): the block's content bytes."""
    b = bytes(frame)
    assert int.from_bytes(b[:4], "little") == 0xFD2FB528
    fhd = b[4]
    single = (fhd >> 5) & 1
    pos = 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3] + [1 if single else 0, 2, 4, 8][fhd >> 6]
    while True:
        bh = b[pos] | b[pos + 1] << 8 | b[pos + 2] << 16
        last, btype, size = bh & 1, (bh >> 1) & 3, bh >> 3
        pos += 3
        assert btype != 3
        if btype < 2:
            pos += size if btype == 0 else 1
            yield btype, (None, size, None, None, 0), pos
        else:
            v = int.from_bytes(b[pos : pos + 5], "little")
            t, fmt = v & 3, (v >> 2) & 3
            if t < 2:
                h = 1 if fmt in (0, 2) else (2 if fmt == 1 else 3)
                regen = (v & ((1 << 8 * h) - 1)) >> (3 if h == 1 else 4)
                cs, tree = (regen if t == 0 else 1), None
            else:
                if fmt < 2:
                    regen, cs, h = (v >> 4) & 0x3FF, (v >> 14) & 0x3FF, 3
                elif fmt == 2:
                    regen, cs, h = (v >> 4) & 0x3FFF, (v >> 18) & 0x3FFF, 4
                else:
                    regen, cs, h = (v >> 4) & 0x3FFFF, (v >> 22) & 0x3FFFF, 5
                tree = None
                if t == 2:
                    hb = b[pos + h]
                    tree = b[pos + h : pos + h + (1 + hb if hb < 128 else 1 + (hb - 127 + 1) // 2)]
            q = pos + h + cs
            n0 = b[q]
            nseq = n0 if n0 < 128 else (b[q + 1] + (b[q + 2] << 8) + 0x7F00 if n0 == 255 else ((n0 - 128) << 8) + b[q + 1])
            pos += size
            yield 2, (t, regen, cs, tree, nseq), pos
        if last:
            return


def weights_from_tree(tree):
    """Huffman code lengths [256] from a tree description (RFC 8878 4.2.1): direct 4-bit weights or FSE-coded weights."""
    t = bytes(tree)
    hb = t[0]
    if hb >= 128:
        nw = hb - 127
        w = []
        for i in range(nw):
            b = t[1 + i // 2]
            w.append(b >> 4 if i % 2 == 0 else b & 15)
    else:
        data = t[1 : 1 + hb]
        val = int.from_bytes(data, "little")
        pos = 0

        def take(k):
            nonlocal pos
            v = (val >> pos) & ((1 << k) - 1)
            pos += k
            return v

        log = take(4) + 5
        remaining, threshold, nbits = (1 << log) + 1, 1 << log, log + 1
        norm, prev0 = [], False
        while remaining > 1 and len(norm) <= 255:
            if prev0:
                while True:
                    r = take(2)
                    norm.extend([0] * r)
                    if r != 3:
                        break
                prev0 = False
                continue
            mx = (2 * threshold - 1) - remaining
            v = (val >> pos) & ((1 << nbits) - 1)
            if (v & (threshold - 1)) < mx:
                c = v & (threshold - 1)
                pos += nbits - 1
            else:
                c = v & (2 * threshold - 1)
                if c >= threshold:
                    c -= mx
                pos += nbits
            c -= 1
            remaining -= abs(c)
            norm.append(c)
            prev0 = c == 0
            while remaining < threshold:
                nbits -= 1
                threshold >>= 1
        assert remaining == 1
        hdr = (pos + 7) // 8
        size = 1 << log
        sym, high = [0] * size, size - 1
        for s, c in enumerate(norm):
            if c == -1:
                sym[high] = s
                high -= 1
        step, p = (size >> 1) + (size >> 3) + 3, 0
        for s, c in enumerate(norm):
            for _ in range(max(c, 0)):
                sym[p] = s
                p = (p + step) & (size - 1)
                while p > high:
                    p = (p + step) & (size - 1)
        nxt = [1 if c == -1 else c for c in norm]
        tab = []
        for u in range(size):
            s = sym[u]
            ns = nxt[s]
            nxt[s] += 1
            nb = log - (ns.bit_length() - 1)
            tab.append((s, nb, (ns << nb) - size))
        stream = int.from_bytes(data[hdr:], "little")
        top = len(data[hdr:]) * 8 - 1
        while not (stream >> top) & 1:
            top -= 1
        bitpos = top  # unread bits are [0, bitpos)
        left = [bitpos]

        def rd(k):
            left[0] -= k
            if left[0] >= 0:
                return (stream >> left[0]) & ((1 << k) - 1)
            have = k + left[0]  # bits that exist; the rest read as zero
            return ((stream & ((1 << max(have, 0)) - 1)) << (k - max(have, 0))) if have > 0 else 0

        s1, s2 = rd(log), rd(log)
        w = []
        while True:
            e = tab[s1]
            w.append(e[0])
            s1 = e[2] + rd(e[1])
            if left[0] < 0:
                w.append(tab[s2][0])
                break
            e = tab[s2]
            w.append(e[0])
            s2 = e[2] + rd(e[1])
            if left[0] < 0:
                w.append(tab[s1][0])
                break
    total = sum((1 << (x - 1)) for x in w if x)
    log2 = total.bit_length()
    rest = (1 << log2) - total
    assert rest and rest & (rest - 1) == 0
    w.append(rest.bit_length())
    nb = np.zeros(256, np.uint8)
    for s, x in enumerate(w):
        nb[s] = log2 + 1 - x if x else 0
    return nb
