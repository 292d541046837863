"""Model-input chunks on the MI355X (include/vbz_gpu.h: vbz_gpu_chunk_layout_batch, vbz_gpu_decompress_chunks_batch; batch.GpuCodec.
chunk_layout, decompress_chunks, decompress_packed_chunks).  The layout is held to a numpy statement of the chunking scheme; every chunk
decode to the int16 decode of the same batch: the same verdict read by read and, where that is a success, every row bit for bit numpy's
chunking of numpy's conversion, pad bits the pad value rounded to the output type."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import oracle_lib as O
from signal_ref import chunk_starts, is_nan_bits, pad_bits, ref_rows, table_of, typed_bits
from typed_support import CANARY, ELEM, arena, codec, compress, device_frames, fmt, i32, key, u32
from vbz_compression_amd import _lib, batch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E_DEST = 0xFFFFFFFC
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
SCHEMES = [(8, 8), (16, 8), (4000, 4000), (4096, 1024), (10000, 9504)]
MODES = [("pad", 0), ("end", 1), ("end", 6), ("end", 8), ("end", 4096)]

def calibration(rng, n):
    return rng.uniform(-600.0, 600.0, n).astype(np.float32), rng.uniform(0.01, 2.5, n).astype(np.float32)


def host_samples(src, src_off, src_size, caps16, sized):
    """T per read as the decoder sees it: unsized, the capacity / 2; sized, the header's size / 2 (0 where there is no header)"""
    if not sized:
        return [int(x) // 2 for x in caps16]
    h = src.cpu().numpy()
    out = []
    for o, s, cap in zip(src_off.cpu().tolist(), u32(src_size).tolist(), caps16):
        hdr = int(h[o : o + 4].view(np.uint32)[0]) if s >= 4 else 0
        out.append(hdr // 2 if hdr <= int(cap) else 0)   # (a header beyond the capacity: refused before the chunk check)
    return out


def decode_chunks_both(c, src, src_off, src_size, caps16, opts, sized, dtype, L, S, mode, end_align, pad=0.0, offset=None, scale=None, signed=True,
                       first=None, rows=None, expect=None, after=None, spare=3):
    """The batch decoded into chunks (the raw entry point, the arena pre-filled with a canary), then to int16 with the capacities caps16 (the
    int16 layout the chunk call was given).  first / rows override the chunk table / chunk_rows; expect[i] the expected verdict.  Checks
    every verdict, every row of every successful read, and that rows of reads the chunk check refused, and rows past the table's total,
    hold the canary.  Returns (chunk results, int16 results, the arena's bits)."""
    dev = c.device
    n = len(caps16)
    dt = key(dtype)
    E = ELEM[dt]
    off16, tot16 = batch.layout([int(x) for x in caps16], 64)
    off16_d = off16.to(dev)
    caps_d = i32(caps16).to(dev)
    Ts = host_samples(src, src_off, src_size, caps16, sized)
    table = table_of(Ts, L, S, mode, end_align) if first is None else np.asarray(first, np.int64)
    total = int(table[-1])
    nrows = total + spare if rows is None else rows
    arena_rows = max(nrows, total) + spare
    chunks = torch.full((arena_rows * L * E,), CANARY, dtype=torch.uint8, device=dev)
    first_d = torch.from_numpy(table).to(dev)
    res = torch.full((n,), -8, dtype=torch.int32, device=dev)
    o_all = np.zeros(n, np.float32) if offset is None else np.asarray(offset, np.float32)
    s_all = np.ones(n, np.float32) if scale is None else np.asarray(scale, np.float32)
    o_d = torch.from_numpy(o_all).to(dev) if offset is not None else None
    s_d = torch.from_numpy(s_all).to(dev) if scale is not None else None
    b = c._batch(src, src_off, src_size, torch.empty(0, dtype=torch.uint8, device=dev), off16_d, caps_d, res)
    b.dst = None
    b.dst_bytes = tot16
    ch = c._chunking(L, S, mode, end_align, pad)
    f = fmt(dtype, signed, o_d, s_d)
    torch.cuda.synchronize()
    rc = c.L.vbz_gpu_decompress_chunks_batch(c.ctx, ctypes.byref(b), ctypes.byref(opts), int(sized), ctypes.byref(f), ctypes.byref(ch), first_d.data_ptr(),
                                             chunks.data_ptr(), nrows)
    assert rc == 0, c.L.vbz_gpu_last_error(c.ctx)
    c.synchronize()
    if after:
        after()
    raw = torch.zeros(tot16 + 64, dtype=torch.uint8, device=dev)
    res16 = torch.full((n,), -8, dtype=torch.int32, device=dev)
    c.decompress(src, src_off, src_size, raw, off16_d, caps_d, res16, opts, sized=sized)
    torch.cuda.synchronize()
    r16, rc_ = u32(res16), u32(res)
    raw_h = raw.cpu().numpy()
    bits = chunks.cpu().numpy().view(np.uint32 if E == 4 else np.uint16).reshape(arena_rows, L)
    padb = pad_bits(pad, dt)
    owned = np.zeros(arena_rows, bool)
    refused = np.zeros(arena_rows, bool)
    offs = off16.tolist()
    for i in range(n):
        want = int(r16[i]) if _lib.is_error(int(r16[i])) else int(r16[i]) // 2 * E
        if expect and i in expect:
            want = expect[i]
        assert int(rc_[i]) == want, (i, hex(int(rc_[i])), hex(want), hex(int(r16[i])))
        lo, hi = int(table[i]), int(table[i + 1])
        if expect and i in expect and expect[i] == E_DEST:   # (refused by the chunk check: nothing written for it)
            refused[max(0, min(lo, hi)) : min(max(lo, hi), arena_rows)] = True
            continue
        if _lib.is_error(want):
            continue
        T = want // E
        x16 = raw_h[offs[i] : offs[i] + 2 * T].view(np.int16 if signed else np.uint16)
        ref = ref_rows(typed_bits(x16, o_all[i], s_all[i], dt), T, L, S, mode, end_align, padb)
        assert hi - lo == ref.shape[0], (i, hi - lo, ref.shape)
        got = bits[lo:hi]
        nan = is_nan_bits(ref, dt)
        bad = (got != ref) & ~nan
        assert not bad.any(), (i, T, np.argwhere(bad)[:4].tolist())
        assert is_nan_bits(got[nan], dt).all(), i
        owned[lo:hi] = True
    assert (bits[refused & ~owned].view(np.uint8) == CANARY).all(), "a row of a read the chunk check refused was written"
    tail = bits[total:]
    assert (tail.view(np.uint8) == CANARY).all(), "a row past the table's total was written"
    return rc_, r16, bits


def lens_for(L, S):
    return [0, 1, 7, 8, L - 1, L, L + 1, L + S - 1, L + S, 100003]


# ---- 1. the layout ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,S", SCHEMES)
def test_layout_matches_numpy(L, S):
    c = codec()
    Ts = [0, 1, 7, 8, L - 1, L, L + 1, L + S - 1, L + S, 100003, (1 << 21) + 5]
    Ts = Ts + [0x80000000, 0xFFFFFFFC] + Ts[::-1]   # (error codes of the size query: no chunks)
    samples = i32(Ts).to(c.device)
    for mode, ea in MODES:
        first, info = c.chunk_layout(samples, L, S, mode=mode, end_align=ea)
        torch.cuda.synchronize()
        Tr = [t if t < 0x80000000 else 0 for t in Ts]
        want = table_of(Tr, L, S, mode, ea)
        assert np.array_equal(first.cpu().numpy(), want), (mode, ea)
        rows = [(i, int(s)) for i, t in enumerate(Tr) for s in chunk_starts(t, L, S, mode, ea)]
        assert np.array_equal(info.cpu().numpy().astype(np.int64), np.array(rows, np.int64).reshape(-1, 2)), (mode, ea)


def test_layout_of_a_million_reads():
    c = codec()
    n = 1 << 20
    rng = np.random.default_rng(5)
    Ts = rng.integers(0, 30000, n)
    Ts[::97] = 0
    L, S = 4096, 1024
    first, info = c.chunk_layout(i32(Ts).to(c.device), L, S, mode="end", end_align=6)
    torch.cuda.synchronize()
    K = np.where(Ts == 0, 0, np.where(Ts <= L, 1, -(-(Ts - L) // S) + 1))
    want = np.zeros(n + 1, np.int64)
    want[1:] = np.cumsum(K)
    assert np.array_equal(first.cpu().numpy(), want)
    inf = info.cpu().numpy()
    assert np.array_equal(inf[:, 0], np.repeat(np.arange(n), K))
    for i in (1, 2, 3, n // 2 + 1, n - 1):   # (a few reads' starts in full)
        lo, hi = want[i], want[i + 1]
        assert np.array_equal(inf[lo:hi, 1], chunk_starts(int(Ts[i]), L, S, "end", 6)), i


def test_layout_leaves_a_small_info_untouched():
    c = codec()
    dev = c.device
    Ts = [100, 5000, 20000]
    samples = i32(Ts).to(dev)
    first = torch.empty(4, dtype=torch.int64, device=dev)
    ch = c._chunking(1024, 512, "pad", 0, 0.0)
    total = int(table_of(Ts, 1024, 512, "pad", 0)[-1])
    info = torch.full((total + 4, 2), -3, dtype=torch.int32, device=dev)
    assert c.L.vbz_gpu_chunk_layout_batch(c.ctx, 3, samples.data_ptr(), ctypes.byref(ch), first.data_ptr(), info.data_ptr(), total - 1) == 0
    c.synchronize()
    assert int(first[-1]) == total
    assert (info == -3).all(), "chunk_info written although the total exceeds info_cap"
    assert c.L.vbz_gpu_chunk_layout_batch(c.ctx, 3, samples.data_ptr(), ctypes.byref(ch), first.data_ptr(), info.data_ptr(), total) == 0
    c.synchronize()
    assert (info[total:] == -3).all()
    assert (info[:total, 0].cpu().numpy() == np.repeat(np.arange(3), np.diff(table_of(Ts, 1024, 512, "pad", 0)))).all()


# ---- 2. content: the option grid ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sized", [False, True])
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("version", [0, 1])
@pytest.mark.parametrize("zz", [True, False])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_bit_exact_grid(dtype, zz, version, level, sized):
    c = codec()
    rng = np.random.default_rng(version * 8 + level * 4 + sized * 2 + zz)
    opts = c.options(zz, 2, level, version)
    for si, (L, S) in enumerate(SCHEMES):
        lens = lens_for(L, S)
        if zz:
            reads = [O.synth_signal(3, i, x) for i, x in enumerate(lens)]
        else:
            reads = [rng.integers(0, 1 << 16, x).astype(np.uint16) for x in lens]
        src, off, size = compress(c, reads, opts, sized)
        caps = [a.nbytes + (2 * int(rng.integers(0, 40)) if sized else 0) for a in reads]
        o, s = calibration(rng, len(reads))
        for mi, (mode, ea) in enumerate(MODES):
            pad = [0.0, -1.5, 3.3, 65519.0, float("inf")][(si + mi) % 5]
            rc, _, _ = decode_chunks_both(c, src, off, size, caps, opts, sized, dtype, L, S, mode, ea, pad=pad, offset=o, scale=s, signed=zz)
            assert int(rc[0]) == 0   # (T = 0: no rows, result 0)
        decode_chunks_both(c, src, off, size, caps, opts, sized, dtype, L, S, "end", 1, signed=zz)   # NULL tables: the identity


# ---- 3. every decode path -----------------------------------------------------------------------------------------------------
def _ragged(rng, n, lo, hi):
    return rng.integers(lo, hi, n).tolist()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_many_reads_and_the_split(dtype):
    c = codec()
    n = 16384   # (the batch runs as two halves)
    rng = np.random.default_rng(n)
    lens = _ragged(rng, n, 1, 6000)
    opts = c.options(True, 2, 1, 1)
    src, off, size = device_frames(c, lens, 11, opts)
    o, s = calibration(rng, n)
    for L, S, mode, ea in ((800, 760, "end", 1), (1024, 512, "pad", 0)):
        decode_chunks_both(c, src, off, size, [2 * x for x in lens], opts, False, dtype, L, S, mode, ea, pad=-2.0, offset=o, scale=s)


@pytest.mark.parametrize("sized", [False, True])
def test_routed_long_reads(sized):
    c = codec()
    rng = np.random.default_rng(21)
    lens = _ragged(rng, 1200, 500, 5000)
    lens[100] = 300_000   # >= 512 KB: routed to the large-read path beside the rest
    lens[901] = 700_001
    opts = c.options(True, 2, 1, 1)
    src, off, size = device_frames(c, lens, 12, opts, sized)
    o, s = calibration(rng, len(lens))
    for dtype, (L, S, mode, ea) in ((torch.float16, (10000, 9504, "end", 1)), (torch.bfloat16, (4096, 1024, "end", 6)),
                                    (torch.float32, (4000, 4000, "pad", 0))):
        decode_chunks_both(c, src, off, size, [2 * x for x in lens], opts, sized, dtype, L, S, mode, ea, pad=1.0, offset=o, scale=s)


def test_one_large_read_on_the_span_path():
    c = codec()
    opts = c.options(True, 2, 1, 1)
    src, off, size = device_frames(c, [4_000_003], 13, opts)
    for dtype, (L, S, mode, ea) in ((torch.float16, (10000, 9504, "end", 1)), (torch.float32, (4096, 1024, "pad", 0)),
                                    (torch.bfloat16, (16, 8, "end", 6))):
        paths = []
        decode_chunks_both(c, src, off, size, [8_000_006], opts, False, dtype, L, S, mode, ea, offset=[-37.5], scale=[0.173],
                           after=lambda: paths.append(c.decode_span_paths()))
        assert paths == [(1, 1)], paths


@pytest.mark.parametrize("segmented", ["1", "0"])
def test_forced_paths_in_fresh_contexts(segmented):
    old = os.environ.get("VBZ_HIP_SEGMENTED")
    os.environ["VBZ_HIP_SEGMENTED"] = segmented
    try:
        c = batch.GpuCodec(0)
    finally:
        if old is None:
            del os.environ["VBZ_HIP_SEGMENTED"]
        else:
            os.environ["VBZ_HIP_SEGMENTED"] = old
    rng = np.random.default_rng(31)
    lens = [0, 1, 9, 4097] + _ragged(rng, 60, 100, 40000) + [600_001]
    for level in (0, 1):
        opts = c.options(True, 2, level, 1)
        src, off, size = device_frames(c, lens, 14, opts)
        o, s = calibration(rng, len(lens))
        for dtype, (L, S, mode, ea) in ((torch.float16, (10000, 9504, "end", 1)), (torch.float32, (16, 8, "end", 6)),
                                        (torch.bfloat16, (4096, 1024, "pad", 0))):
            decode_chunks_both(c, src, off, size, [2 * x for x in lens], opts, False, dtype, L, S, mode, ea, pad=7.0, offset=o, scale=s)
    c.close()


def test_frames_libzstd_wrote_are_walked():
    c = batch.GpuCodec(0)   # (a fresh context: it has seen no call without foreign frames)
    rng = np.random.default_rng(41)
    n = 4096
    lens = _ragged(rng, n, 1000, 3000)
    reads = [O.synth_signal(15, i, x) for i, x in enumerate(lens)]
    frames = [O.compress(a, O.options(True, 2, 1, 0)) for a in reads]
    src, off, size = arena(c, frames, 64)
    opts = c.options(True, 2, 1, 0)
    o, s = calibration(rng, n)
    paths = []
    decode_chunks_both(c, src, off, size, [a.nbytes for a in reads], opts, False, torch.float16, 800, 760, "end", 1, offset=o, scale=s,
                       after=lambda: paths.append(c.decode_paths()))
    assert paths[0][0] == n and paths[0][2] == n, paths
    c.close()


def test_fast5_chunks():
    c = codec()
    idx = json.load(open(os.path.join(GOLDEN, "fast5_chunks.json")))
    blob = np.fromfile(os.path.join(GOLDEN, "fast5_chunks.bin"), np.uint8)
    bufs = [blob[e["chunk_offset"] : e["chunk_offset"] + e["chunk_size"]] for e in idx]
    src, off, size = arena(c, bufs, 16)
    opts = c.options(True, 2, 1, 0)
    caps = [2 * e["samples"] for e in idx]
    rc, _, _ = decode_chunks_both(c, src, off, size, caps, opts, True, torch.float16, 4000, 3600, "end", 8)
    assert [int(r) for r in rc] == [e["samples"] * 2 for e in idx]


def test_checksummed_frames():
    c = codec()
    c.set_checksum(True)
    try:
        rng = np.random.default_rng(61)
        lens = _ragged(rng, 500, 1, 20000)
        opts = c.options(True, 2, 1, 1)
        src, off, size = device_frames(c, lens, 16, opts)
    finally:
        c.set_checksum(False)
    o, s = calibration(rng, len(lens))
    for dtype in DTYPES:
        decode_chunks_both(c, src, off, size, [2 * x for x in lens], opts, False, dtype, 2000, 1800, "end", 1, offset=o, scale=s)


# ---- 4. verdicts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_damaged_frames_give_the_int16_verdicts(dtype):
    c = codec()
    rng = np.random.default_rng(71)
    lens = _ragged(rng, 300, 1, 9000)
    reads = [O.synth_signal(17, i, x) for i, x in enumerate(lens)]
    for sized, checksum in ((False, False), (True, False), (False, True)):
        opts = c.options(True, 2, 1, 1)
        c.set_checksum(checksum)
        try:
            src, off, size = compress(c, reads, opts, sized)
        finally:
            c.set_checksum(False)
        sz = u32(size)
        offs = off.cpu().tolist()
        h = src.cpu().numpy().copy()
        n = len(reads)
        sizes = [int(x) for x in sz]
        for i in range(0, n, 3):   # damage: flipped bytes, truncation, a damaged checksum
            kind = (i // 3) % 3
            if kind == 0 and sizes[i] > 8:
                h[offs[i] + int(rng.integers(4, sizes[i]))] ^= 0xFF
            elif kind == 1 and sizes[i] > 2:
                sizes[i] = int(rng.integers(1, sizes[i]))
            elif sizes[i] > 8:
                h[offs[i] + sizes[i] - 1] ^= 0x01
        dsrc = torch.from_numpy(h).to(c.device)
        caps = [a.nbytes for a in reads]
        if sized:
            for i in range(1, n, 7):   # a capacity too small for the header's size
                caps[i] = max(0, caps[i] - 2)
        decode_chunks_both(c, dsrc, off, i32(sizes).to(c.device), caps, opts, sized, dtype, 1000, 952, "end", 1)


def test_fuzz_corpus_verdicts():
    c = codec()
    idx = json.load(open(os.path.join(GOLDEN, "fuzz_corpus.json")))
    blob = np.fromfile(os.path.join(GOLDEN, "fuzz_corpus.bin"), np.uint8)
    files = [blob[e["offset"] : e["offset"] + e["size"]] for e in idx][:120]
    bufs, caps = [], []
    for f in files:   # every file at a few guessed destination sizes
        for cap in (0, 2, 64, 2 * f.nbytes, 8 * f.nbytes):
            bufs.append(f)
            caps.append(cap)
    src, off, size = arena(c, bufs, 64)
    for zz, level, version in ((True, 1, 0), (False, 1, 1), (True, 0, 1)):
        opts = c.options(zz, 2, level, version)
        for sized in (False, True):
            decode_chunks_both(c, src, off, size, caps, opts, sized, torch.float16, 64, 40, "end", 6, signed=zz)


# ---- 5. canaries: the untrusted table ---------------------------------------------------------------------------------------
def _table_batch(c):
    lens = [5000, 12345, 801, 9000, 3, 40000, 7777]
    reads = [O.synth_signal(22, i, x) for i, x in enumerate(lens)]
    opts = c.options(True, 2, 1, 1)
    src, off, size = compress(c, reads, opts)
    return lens, reads, opts, src, off, size


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_wrong_table_entries_write_nothing(dtype):
    c = codec()
    lens, reads, opts, src, off, size = _table_batch(c)
    caps = [a.nbytes for a in reads]
    L, S = 1000, 904
    good = table_of(lens, L, S, "end", 1)
    # read 2 one row short (read 3 one row long), read 5 one row long (read 6 one row short)
    t = good.copy()
    t[3] -= 1
    t[6] += 1
    decode_chunks_both(c, src, off, size, caps, opts, False, dtype, L, S, "end", 1, pad=9.0, first=t,
                       expect={2: E_DEST, 3: E_DEST, 5: E_DEST, 6: E_DEST})
    # a decreasing entry
    t = good.copy()
    t[4] = t[5] + 1
    decode_chunks_both(c, src, off, size, caps, opts, False, dtype, L, S, "end", 1, first=t, expect={3: E_DEST, 4: E_DEST})
    # the last read past chunk_rows (one row short of the table's total); nothing beyond chunk_rows is written either
    decode_chunks_both(c, src, off, size, caps, opts, False, dtype, L, S, "end", 1, rows=int(good[-1]) - 1, expect={6: E_DEST})


def test_empty_read_writes_nothing():
    c = codec()
    reads = [np.zeros(0, np.int16), O.synth_signal(23, 1, 100), np.zeros(0, np.int16)]
    opts = c.options(True, 2, 1, 1)
    src, off, size = compress(c, reads, opts)
    rc, _, bits = decode_chunks_both(c, src, off, size, [0, 200, 0], opts, False, torch.float16, 256, 256, "pad", 0, pad=0.5, spare=2)
    assert [int(r) for r in rc] == [0, 200, 0]
    assert (bits[1:].view(np.uint8) == CANARY).all()   # (one row: read 1; nothing else)


# ---- 6. host refusals ------------------------------------------------------------------------------------------------------
def test_host_refusals():
    c = codec()
    dev = c.device
    L_ = c.L
    reads = [O.synth_signal(19, 0, 1000)]
    opts = c.options(True, 2, 1, 1)
    src, off, size = compress(c, reads, opts)
    doff = torch.zeros(1, dtype=torch.int64, device=dev)
    dcap = i32([2000]).to(dev)
    res = torch.full((1,), -8, dtype=torch.int32, device=dev)
    first = torch.tensor([0, 1], dtype=torch.int64, device=dev)
    chunks = torch.full((4096 + 16,), CANARY, dtype=torch.uint8, device=dev)

    def batch_():
        b = c._batch(src, off, size, torch.empty(0, dtype=torch.uint8, device=dev), doff, dcap, res)
        b.dst = None
        b.dst_bytes = 2000
        return b

    def call(o=opts, f="ok", ch="ok", bt="ok", fp="ok", cp="ok", rows=1):
        f = fmt(torch.float16, True) if f == "ok" else f
        ch = c._chunking(1024, 1024, "pad", 0, 0.0) if ch == "ok" else ch
        bt = batch_() if bt == "ok" else bt
        fp = first.data_ptr() if fp == "ok" else fp
        cp = chunks.data_ptr() if cp == "ok" else cp
        return L_.vbz_gpu_decompress_chunks_batch(c.ctx, ctypes.byref(bt) if bt is not None else None, ctypes.byref(o) if o is not None else None, 0,
                                                  ctypes.byref(f) if f is not None else None, ctypes.byref(ch) if ch is not None else None, fp, cp,
                                                  rows)

    def bad_ch(**kw):
        ch = c._chunking(1024, 512, "end", 1, 0.0)
        for k, v in kw.items():
            setattr(ch, k, v)
        return ch

    for isz, ver in ((1, 1), (4, 1), (0, 1), (2, 2)):
        assert call(o=c.options(True, isz, 1, ver)) == -2, (isz, ver)
    assert call(o=None) == -2
    assert call(f=None) == -2
    for t, sg in ((0, 1), (4, 1), (1, 2)):
        f = _lib.GpuSignalFormat()
        f.out_type, f.is_signed = t, sg
        assert call(f=f) == -2, (t, sg)
    assert call(ch=None) == -2
    for kw in ({"chunk_len": 0}, {"chunk_len": 12}, {"chunk_len": (1 << 20) + 8}, {"step": 0}, {"step": 4}, {"step": 1028}, {"step": 2048},
               {"mode": 2}, {"end_align": 0}, {"end_align": 4097}, {"reserved": 1}):
        assert call(ch=bad_ch(**kw)) == -2, kw
    pad_mode = c._chunking(1024, 512, "pad", 0, 0.0)
    pad_mode.end_align = 1
    assert call(ch=pad_mode) == -2
    assert call(fp=None) == -2
    assert call(cp=None) == -2
    assert call(cp=chunks.data_ptr() + 8) == -2   # misaligned
    assert call(rows=(1 << 46) // 2048 + 1) == -2   # an oversized extent
    bad = batch_()
    bad.src_off = None
    assert call(bt=bad) == -2
    big = batch_()
    big.dst_bytes = (1 << 46) + 1
    assert call(bt=big) == -2
    assert L_.vbz_gpu_chunk_layout_batch(c.ctx, 1, None, ctypes.byref(pad_mode), first.data_ptr(), None, 0) == -2
    assert L_.vbz_gpu_chunk_layout_batch(c.ctx, 1, dcap.data_ptr(), ctypes.byref(bad_ch(step=4)), first.data_ptr(), None, 0) == -2
    assert L_.vbz_gpu_chunk_layout_batch(c.ctx, 1, dcap.data_ptr(), ctypes.byref(bad_ch()), None, None, 0) == -2
    torch.cuda.synchronize()
    assert int(res[0]) == -8, "nothing was launched"
    assert (chunks == CANARY).all()
    assert int(first[1]) == 1
    assert L_.vbz_gpu_decompress_chunks_batch(c.ctx, None, ctypes.byref(opts), 0, ctypes.byref(fmt(torch.float16, True)),
                                              ctypes.byref(c._chunking(1024, 1024, "pad", 0, 0.0)), first.data_ptr(), chunks.data_ptr(), 1) == -1
    assert call() == 0
    torch.cuda.synchronize()
    assert int(res[0]) == 2000


# ---- 7. Python round trip --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,ea", [("pad", 0), ("end", 1), ("end", 6)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_packed_round_trip(dtype, mode, ea):
    c = codec()
    rng = np.random.default_rng(91)
    lens = [0, 1, 17] + _ragged(rng, 200, 100, 60000) + [300_000]
    reads = [O.synth_signal(20, i, x) for i, x in enumerate(lens)]
    opts = c.options(True, 2, 1, 1)
    comp, coff, res = compress(c, reads, opts, sized=True)
    caps = [c.L.vbz_max_compressed_size(int(a.nbytes), ctypes.byref(opts)) for a in reads]
    packed, poff, psize = c.pack(comp, coff, i32(caps).to(c.device), res, align=16)
    o, s = calibration(rng, len(reads))
    od, sd = torch.from_numpy(o).to(c.device), torch.from_numpy(s).to(c.device)
    L, S = 4000, 3000
    chunks, first, info, result = c.decompress_packed_chunks(packed, poff, psize, opts, L, S, mode=mode, end_align=ea, pad=-0.25, dtype=dtype,
                                                             offset=od, scale=sd)
    out, out_off, samples, result_s = c.decompress_packed_signal(packed, poff, psize, opts, dtype=dtype, offset=od, scale=sd)
    torch.cuda.synchronize()
    assert torch.equal(result, result_s)
    # the unfused route: one gather through the flat index of the layout
    starts = info[:, 1].to(torch.int64)
    rd = info[:, 0].to(torch.int64)
    pos = starts[:, None] + torch.arange(L, device=c.device)[None, :]
    inside = pos < samples.to(torch.int64)[rd][:, None]
    flat = out_off[rd][:, None] + torch.where(inside, pos, torch.zeros_like(pos))
    want = torch.where(inside, out[flat], torch.full_like(out[flat], -0.25))
    assert chunks.dtype == dtype and chunks.shape == (int(first[-1]), L)
    assert torch.equal(chunks.view(torch.int16 if ELEM[key(dtype)] == 2 else torch.int32), want.view(torch.int16 if ELEM[key(dtype)] == 2 else torch.int32))
    assert int(first[-1]) == int(table_of(lens, L, S, mode, ea)[-1])


def test_unsized_python_call():
    c = codec()
    rng = np.random.default_rng(93)
    lens = [0, 5, 9999, 10000, 10001] + _ragged(rng, 100, 1, 40000)
    opts = c.options(True, 2, 1, 1)
    src, off, size = device_frames(c, lens, 24, opts)
    samples = i32(lens).to(c.device)
    result = torch.empty(len(lens), dtype=torch.int32, device=c.device)
    chunks, first, info = c.decompress_chunks(src, off, size, samples, result, opts, 10000, 9504, mode="end", end_align=1)
    torch.cuda.synchronize()
    assert [int(r) for r in result.cpu()] == [2 * x for x in lens]
    assert np.array_equal(first.cpu().numpy(), table_of(lens, 10000, 9504, "end", 1))
    assert chunks.shape == (int(first[-1]), 10000) and chunks.dtype == torch.float16
    # against the signal decode of the same batch
    off16, tot16 = batch.layout([2 * x for x in lens], 16)
    out = torch.empty(tot16 // 2, dtype=torch.float16, device=c.device)
    res2 = torch.empty_like(result)
    c.decompress_signal(src, off, size, out, off16.to(c.device), i32([2 * x for x in lens]).to(c.device), res2, opts)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    h = chunks.cpu().numpy()
    for i, t in enumerate(lens):
        rows = ref_rows(o[int(off16[i]) // 2 : int(off16[i]) // 2 + t].view(np.uint16), t, 10000, 9504, "end", 1, 0)
        assert np.array_equal(h[int(first[i]) : int(first[i + 1])].view(np.uint16), rows), i
