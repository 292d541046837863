"""CPU tests of vbz_compression_amd/csrc/zstd_frame.h, the header readers every zstd decoder of the library calls: frame headers against
libzstd's own ZSTD_getFrameHeader, block walks against libzstd's bufferless decoder, literals and sequences section headers against the
oracle's restatement (oracle/zstd_restate.c), the checkpoint / span index trailers and the skippable-frame walk against the layout the
encoder writes and libzstd's ZSTD_findFrameCompressedSize -- on frames of libzstd and of the library's serial encoder statement, every FHD
byte and every first byte of a section with random bytes behind it, truncated and damaged copies."""
import ctypes
import struct

import numpy as np

import entropy_host as E
import oracle_lib as O

CONTENTSIZE_UNKNOWN = (1 << 64) - 1
ZSTD_MAGIC, SKIP_MAGIC, CP_MAGIC, IDX_MAGIC = 0xFD2FB528, 0x184D2A50, 0x184D2A5B, 0x184D2A5C


class _FrameHeader(ctypes.Structure):   # ZSTD_frameHeader (libzstd 1.4 / 1.5), with room to spare
    _fields_ = [("frameContentSize", ctypes.c_ulonglong), ("windowSize", ctypes.c_ulonglong), ("blockSizeMax", ctypes.c_uint),
                ("frameType", ctypes.c_int), ("headerSize", ctypes.c_uint), ("dictID", ctypes.c_uint), ("checksumFlag", ctypes.c_uint),
                ("_reserved", ctypes.c_uint * 8)]


def _z():
    Z = O.libzstd()
    Z.ZSTD_getFrameHeader.restype = ctypes.c_size_t
    Z.ZSTD_getFrameHeader.argtypes = [ctypes.POINTER(_FrameHeader), ctypes.c_void_p, ctypes.c_size_t]
    Z.ZSTD_findFrameCompressedSize.restype = ctypes.c_size_t
    Z.ZSTD_findFrameCompressedSize.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    return Z


def _arr(b, pad=0):
    return np.frombuffer(bytes(b) + bytes(pad), np.uint8).copy()


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def dev_frame_header(b, n=None):
    n = len(b) if n is None else n
    a = _arr(b[:n])
    out = np.zeros(8, np.uint32)
    big = np.zeros(2, np.uint64)
    whole = E.lib().h_frame_header(_ptr(a), n, _ptr(out), _ptr(big))
    keys = ("magic", "fhd", "len", "wlog", "did_bytes", "did", "fcs_bytes", "checksum")
    h = dict(zip(keys, (int(x) for x in out)))
    h["fcs"], h["window"] = int(big[0]), int(big[1])
    return bool(whole), h


def check_frame_header(b):
    """The device's reading of the header at the start of b against ZSTD_getFrameHeader's."""
    Z = _z()
    a = _arr(b)
    zh = _FrameHeader()
    r = Z.ZSTD_getFrameHeader(ctypes.byref(zh), _ptr(a), len(b))
    whole, h = dev_frame_header(b)
    assert h["magic"] == ZSTD_MAGIC
    assert h["fhd"] == b[4] and h["checksum"] == (b[4] >> 2) & 1
    if Z.ZSTD_isError(r):
        # libzstd's refusals: the reserved bit, a window log above 31 -- the device refuses both at its call sites
        assert whole and ((h["fhd"] & 8) or h["wlog"] > 31), (b[:18].hex(), h)
        return h
    if r > 0:   # libzstd needs r bytes
        assert not whole and h["len"] == r, (b[:18].hex(), r, h)
        return h
    assert whole and not (h["fhd"] & 8) and h["wlog"] <= 31, h
    assert h["len"] == zh.headerSize
    assert h["checksum"] == zh.checksumFlag
    assert h["did"] == zh.dictID
    assert h["did_bytes"] == (0, 1, 2, 4)[b[4] & 3]
    if h["fcs_bytes"] == 0:   # no content size: the device refuses such frames
        assert zh.frameContentSize == CONTENTSIZE_UNKNOWN
    else:
        assert h["fcs"] == zh.frameContentSize
    assert h["window"] == zh.windowSize, (b[:18].hex(), h, zh.windowSize)
    return h


def dev_block_walk(f, pos):
    """(block header offsets, where the last block ends) by zstd_block_header; None if a header runs past the buffer"""
    heads, out = [], np.zeros(4, np.uint32)
    while True:
        if pos + 3 > len(f):
            return None
        E.lib().h_block_header.argtypes = [ctypes.c_uint32, ctypes.c_void_p]
        E.lib().h_block_header(f[pos] | f[pos + 1] << 8 | f[pos + 2] << 16 | 0xAB000000, _ptr(out))
        last, typ, size, src = (int(x) for x in out)
        assert (last, typ, size) == (f[pos] & 1, (f[pos] >> 1) & 3, (f[pos] | f[pos + 1] << 8 | f[pos + 2] << 16) >> 3)
        heads.append(pos)
        pos += 3 + src
        if pos > len(f):
            return None
        if last:
            return heads, pos


def libzstd_block_walk(f, cap):
    """The same by libzstd's bufferless decoder: where it reads every block header, and where the blocks end."""
    Z = O.libzstd()
    a = _arr(f)
    dst = np.zeros(max(cap, 1), np.uint8)
    dc = Z.ZSTD_createDCtx()
    heads, ipos, opos = [], 0, 0
    try:
        assert not Z.ZSTD_isError(Z.ZSTD_decompressBegin(dc))
        while True:
            need = Z.ZSTD_nextSrcSizeToDecompress(dc)
            kind = Z.ZSTD_nextInputType(dc)   # ZSTDnit_blockHeader = 1, checksum = 4
            if need == 0 or kind == 4:
                return heads, ipos
            if kind == 1:
                heads.append(ipos)
            r = Z.ZSTD_decompressContinue(dc, dst.ctypes.data + opos, len(dst) - opos, a.ctypes.data + ipos, need)
            assert not Z.ZSTD_isError(r)
            ipos += need
            opos += r
    finally:
        Z.ZSTD_freeDCtx(dc)


def dev_lit_header(v8):
    out = np.zeros(6, np.uint32)
    E.lib().h_lit_header(ctypes.c_uint64(int.from_bytes(bytes(v8[:8]).ljust(8, b"\0"), "little")), _ptr(out))
    return dict(zip(("type", "fmt", "hsize", "regen", "csize", "streams"), (int(x) for x in out)))


def check_lit_header(sec):
    """The device's literals header of the section bytes sec against the oracle's (which also says when sec is too short for it)."""
    a = _arr(sec, 8)
    o = np.zeros(4, np.uint32)
    hs = O.lib().vbo_debug_lit_header(_ptr(a), len(sec), _ptr(o))
    d = dev_lit_header(a)
    assert d["fmt"] == (sec[0] >> 2) & 3
    if hs < 0:
        assert d["hsize"] > len(sec)
        return d
    assert (d["hsize"], d["type"], d["regen"], d["csize"], d["streams"]) == (hs, *(int(x) for x in o)), (bytes(sec[:5]).hex(), d)
    return d


def check_nseq(sec, n):
    a = _arr(sec[:n], 4)
    used, ns = ctypes.c_uint32(0), ctypes.c_uint32(0)
    d = E.lib().h_nseq(_ptr(a), n, ctypes.byref(used))
    r = O.lib().vbo_debug_nseq(_ptr(a), n, ctypes.byref(ns))
    if r < 0:
        assert used.value == 0
    else:
        assert (used.value, d) == (r, ns.value)
    return used.value


def _frames():
    """(frame, content size) from libzstd -- levels, window logs, single segment or not, checksums, flushed blocks, raw and RLE blocks --
    and from the library's serial statement of its zero-run block"""
    rng = np.random.default_rng(5)
    out = []
    for it in range(24):
        n = int(rng.choice([0, 1, 200, 255, 256, 300, 5000, 65791, 65792, 70000, 300000]))
        kind = it % 3
        if kind == 0:
            data = O.svb_compress(O.synth_signal(3, it, max(n // 2, 1)), 2, True, 0)[:n]
        elif kind == 1:
            data = rng.integers(0, 256, n, dtype=np.uint8)
        else:
            data = np.minimum(rng.geometric(0.3, n), 255).astype(np.uint8)
        data = np.ascontiguousarray(data, np.uint8)
        level = int(rng.integers(1, 20))
        wlog = int(rng.choice([0, 10, 12, 17, 20, 27]))
        ck = bool(it & 1)
        out.append((bytes(O.zstd_compress_cuts(data, (), level, wlog, ck)), len(data)))
        if len(data) > 2000:
            cuts = sorted(set(int(c) for c in rng.integers(1, len(data), 4)))
            out.append((bytes(O.zstd_compress_cuts(data, cuts, level, wlog, not ck)), len(data)))
    for lvl in (1, 19):   # constant content: RLE blocks
        out.append((bytes(O.zstd_compress_cuts(np.full(300000, 7, np.uint8), (), lvl, 0, bool(lvl & 1))), 300000))
    for lvl in (1, 3, 9, 19):
        d = O.svb_compress(O.synth_signal(9, lvl, 30000), 2, True, 0)
        out.append((bytes(O.zstd_compress(d, lvl)), len(d)))
    k = np.zeros(40000, np.uint8)
    k[rng.integers(0, 40000, 6000)] = rng.integers(1, 256, 6000)
    buf = np.zeros(1 << 17, np.uint8)
    m = E.lib().h_encode_zero_run_frame(_ptr(k), len(k), _ptr(buf), len(buf), 4)
    assert m > 0
    out.append((bytes(buf[:m]), len(k)))
    return out


FRAMES = None


def frames():
    global FRAMES
    if FRAMES is None:
        FRAMES = _frames()
    return FRAMES


def test_frame_headers_of_real_frames_match_libzstd():
    seen = set()
    for f, n in frames():
        h = check_frame_header(f)
        assert h["fcs_bytes"] and h["fcs"] == n
        seen.add((h["wlog"] == 0, h["checksum"], h["fcs_bytes"]))
        for cut in range(5, h["len"]):   # truncated headers
            check_frame_header(f[:cut])
    assert len(seen) >= 6, seen


def test_every_fhd_byte_matches_libzstd():
    rng = np.random.default_rng(7)
    for fhd in range(256):
        for _ in range(6):
            tail = rng.integers(0, 256, 13, dtype=np.uint8).tobytes()
            b = struct.pack("<IB", ZSTD_MAGIC, fhd) + tail
            h = check_frame_header(b)
            single = (fhd >> 5) & 1
            assert h["len"] == 5 + (1 - single) + (0, 1, 2, 4)[fhd & 3] + ((1 if single else 0), 2, 4, 8)[fhd >> 6]
            for cut in range(5, len(b)):
                check_frame_header(b[:cut])


def test_block_walks_match_libzstd():
    for f, n in frames():
        whole, h = dev_frame_header(f)
        heads, end = dev_block_walk(f, h["len"])
        zheads, zend = libzstd_block_walk(f, n)
        assert heads == zheads and end == zend
        ends = O.zstd_block_ends(f, n)
        assert ends is not None and (len(ends) == len(heads) or n == 0)   # (an empty frame's one block has no content to hand over)
        assert end + 4 * h["checksum"] == len(f)


def test_literals_and_sequences_headers_match_the_oracle():
    rng = np.random.default_rng(3)
    for b0 in range(256):
        for _ in range(8):
            sec = bytes([b0]) + rng.integers(0, 256, 7, dtype=np.uint8).tobytes()
            for n in (1, 2, 3, 4, 5, 8):
                check_lit_header(sec[:n])
                check_nseq(sec, min(n, 4))
    nblk = 0
    for f, n in frames():
        whole, h = dev_frame_header(f)
        heads, end = dev_block_walk(f, h["len"])
        for p in heads:
            bh = f[p] | f[p + 1] << 8 | f[p + 2] << 16
            if (bh >> 1) & 3 != 2:
                continue
            blk = f[p + 3 : p + 3 + (bh >> 3)]
            d = check_lit_header(blk)
            sq = d["hsize"] + d["csize"]
            assert sq < len(blk)
            assert check_nseq(blk[sq:], len(blk) - sq) > 0
            nblk += 1
    assert nblk > 30


def test_huffman_description_sizes():
    rng = np.random.default_rng(2)
    assert E.lib().h_huf_desc_size(0) == 0
    for hb in range(1, 256):
        assert E.lib().h_huf_desc_size(hb) == (1 + hb if hb < 128 else 1 + (hb - 126) // 2)
    for it in range(30):
        t = E.tree_description(np.minimum(rng.geometric(rng.uniform(0.02, 0.5), 20000), 255).astype(np.uint8))[2]
        used = ctypes.c_int(0)
        a = _arr(t)
        assert O.lib().vbo_debug_huf_lengths(_ptr(a), len(t), _ptr(np.zeros(256, np.uint8)), ctypes.byref(used)) >= 0
        assert E.lib().h_huf_desc_size(t[0]) == used.value == len(t)


def _cp_trailer(spacing, words):
    tb = 16 + 4 * len(words)
    return struct.pack("<III", CP_MAGIC, tb - 8, spacing | len(words) << 16) + struct.pack("<%dI" % len(words), *words) + struct.pack("<I", tb)


def _idx_trailer(spans):
    tb = 16 + 8 * len(spans)
    body = b"".join(struct.pack("<II", a, c) for a, c in spans)
    return struct.pack("<III", IDX_MAGIC, tb - 8, len(spans)) + body + struct.pack("<I", tb)


def _expect_checkpoints(b):
    """The trailer rules restated: an index trailer may end the buffer, a checkpoint trailer ends what is in front of it."""
    n = len(b)
    if n < 64:
        return (0, 0, 0)
    w = lambda o: struct.unpack_from("<I", b, o)[0]
    tb, ne = w(n - 4), n
    if 24 <= tb <= n - 16 and tb % 8 == 0 and w(n - tb) == IDX_MAGIC and w(n - tb + 4) == tb - 8:
        ne = n - tb
        tb = w(ne - 4)
    if 20 <= tb <= 8 + 4 + 4 * 63 + 4 and tb + 16 <= ne:
        m0, m1, m2 = w(ne - tb), w(ne - tb + 4), w(ne - tb + 8)
        cnt = m2 >> 16
        if m0 == CP_MAGIC and m1 == tb - 8 and tb == 16 + 4 * cnt and cnt >= 1:
            return (ne - tb + 12, cnt, m2 & 0xFFFF)
    return (0, 0, 0)


def _dev_checkpoints(b):
    a = _arr(b)
    out = np.zeros(3, np.uint32)
    E.lib().h_checkpoints(_ptr(a), len(b), _ptr(out))
    return tuple(int(x) for x in out)


def _libzstd_skip_end(b, pos):
    Z = _z()
    a = _arr(b)
    while len(b) - pos >= 8 and (struct.unpack_from("<I", b, pos)[0] & 0xFFFFFFF0) == SKIP_MAGIC:
        r = Z.ZSTD_findFrameCompressedSize(a.ctypes.data + pos, len(b) - pos)
        if Z.ZSTD_isError(r):
            break
        pos += r
    return pos


def test_trailers_and_skippable_frames():
    rng = np.random.default_rng(4)
    cases = 0
    for f, n in frames():
        whole, h = dev_frame_header(f)
        _, end = dev_block_walk(f, h["len"])
        fend = end + 4 * h["checksum"]
        for with_cp in (False, True):
            for with_idx in (False, True):
                cnt = int(rng.integers(1, 64))
                spacing = int(rng.integers(32, 4096))
                cp = _cp_trailer(spacing, [int(x) for x in rng.integers(0, 1 << 32, cnt, dtype=np.uint64)]) if with_cp else b""
                idx = _idx_trailer([(int(a), int(c)) for a, c in rng.integers(0, 1 << 20, (int(rng.integers(2, 9)), 2))]) if with_idx else b""
                b = bytes(f) + cp + idx
                got = _dev_checkpoints(b)
                assert got == _expect_checkpoints(b)
                if with_cp and len(b) >= 64 and len(f) >= 16:   # (a checkpoint trailer is looked for behind 16 bytes at least)
                    assert got == (len(f) + 12, cnt, spacing)
                elif not with_cp:
                    assert got[1] == 0
                assert E.lib().h_skip_frames(_ptr(_arr(b)), fend, len(b)) == len(b) == _libzstd_skip_end(b, fend)
                # damaged copies: bytes of the trailers overwritten, the buffer cut short, garbage behind it
                for _ in range(12):
                    d = bytearray(b)
                    what = int(rng.integers(0, 3))
                    if what == 0 and len(d) > fend:
                        for _ in range(int(rng.integers(1, 3))):
                            d[int(rng.integers(fend, len(d)))] = int(rng.integers(0, 256))
                    elif what == 1:
                        d = d[: int(rng.integers(fend, len(d) + 1))]
                    else:
                        d += rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
                    d = bytes(d)
                    assert _dev_checkpoints(d) == _expect_checkpoints(d)
                    assert E.lib().h_skip_frames(_ptr(_arr(d, 8)), fend, len(d)) == _libzstd_skip_end(d, fend)
                    cases += 1
    assert cases > 1000
