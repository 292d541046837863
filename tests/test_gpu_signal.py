"""Calibrated signal on the MI355X (include/vbz_gpu.h: vbz_gpu_decompress_signal_batch; batch.GpuCodec.decompress_signal,
decompress_packed_signal).  Every typed decode is held to the int16 decode of the same batch: the same verdict read by read, and
where that is a success, samples bit for bit numpy's ((float32)x + offset) * scale, rounded once more to float16 / bfloat16."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import oracle_lib as O
from signal_ref import typed_bits
from typed_support import ELEM, arena, codec, compress, decode_both, device_frames, i32, key, u32
from vbz_compression_amd import _lib, batch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U32 = 0xFFFFFFFF
E_ZSTD, E_INPUT, E_DEST = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFC
DTYPES = [torch.float32, torch.float16, torch.bfloat16]


def calibration(rng, n, overflow=True):
    o = rng.uniform(-600.0, 600.0, n).astype(np.float32)
    s = rng.uniform(0.01, 2.5, n).astype(np.float32)
    if overflow and n >= 3:
        s[1] = np.float32(1e5)     # float16 / bfloat16: |y| beyond 65504 -> inf (bfloat16 holds it)
        s[2] = np.float32(3e38)    # float32 overflow -> inf
    return o, s


# ---- 1. bit-exact against numpy over the whole option grid -------------------------------------------------------------------
LENS = [0, 1, 7, 8, 2047, 2051, 100003]


@pytest.mark.parametrize("sized", [False, True])
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("version", [0, 1])
@pytest.mark.parametrize("zz", [True, False])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_bit_exact_grid(dtype, zz, version, level, sized):
    c = codec()
    rng = np.random.default_rng(version * 8 + level * 4 + sized * 2 + zz)
    if zz:   # int16 signal (zig-zag on)
        reads = [O.synth_signal(3, i, n) for i, n in enumerate(LENS)]
    else:    # uint16 samples over the whole range (zig-zag off)
        reads = [rng.integers(0, 1 << 16, n).astype(np.uint16) for n in LENS]
    opts = c.options(zz, 2, level, version)
    src, off, size = compress(c, reads, opts, sized)
    caps = [a.nbytes + (2 * int(rng.integers(0, 40)) if sized else 0) for a in reads]
    o, s = calibration(rng, len(reads))
    decode_both(c, src, off, size, caps, opts, sized, dtype, offset=o, scale=s, signed=zz)
    decode_both(c, src, off, size, caps, opts, sized, dtype, signed=zz)   # NULL tables: the identity


def test_nan_constants_give_nan():
    c = codec()
    reads = [O.synth_signal(4, i, 5000) for i in range(3)]
    opts = c.options(True, 2, 1, 1)
    src, off, size = compress(c, reads, opts)
    o = np.array([0.0, np.nan, 1.0], np.float32)
    s = np.array([np.nan, 1.0, 2.0], np.float32)
    for dtype in DTYPES:
        decode_both(c, src, off, size, [a.nbytes for a in reads], opts, False, dtype, offset=o, scale=s)


# ---- 2. every decode path --------------------------------------------------------------------------------------------------
def _ragged(rng, n, lo, hi):
    return rng.integers(lo, hi, n).tolist()


@pytest.mark.parametrize("n", [4096, 16384])   # 16 384: the batch runs as two halves
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_many_reads_and_the_split(n, dtype):
    c = codec()
    rng = np.random.default_rng(n)
    lens = _ragged(rng, n, 1, 6000)
    opts = c.options(True, 2, 1, 1)
    src, off, size = device_frames(c, lens, 11, opts)
    o, s = calibration(rng, n)
    decode_both(c, src, off, size, [2 * x for x in lens], opts, False, dtype, offset=o, scale=s)


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
    for dtype in DTYPES:
        decode_both(c, src, off, size, [2 * x for x in lens], opts, sized, dtype, offset=o, scale=s)


def test_one_large_read_on_the_span_path():
    c = codec()
    opts = c.options(True, 2, 1, 1)
    src, off, size = device_frames(c, [4_000_000], 13, opts)
    for dtype in DTYPES:
        paths = []
        decode_both(c, src, off, size, [8_000_000], opts, False, dtype, offset=[-37.5], scale=[0.173],
                    after_typed=lambda: paths.append(c.decode_span_paths()))
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
    lens = [0, 1, 9, 4097] + _ragged(rng, 60, 100, 40000) + [600_000]
    for level in (0, 1):
        opts = c.options(True, 2, level, 1)
        src, off, size = device_frames(c, lens, 14, opts)
        o, s = calibration(rng, len(lens))
        for dtype in DTYPES:
            decode_both(c, src, off, size, [2 * x for x in lens], opts, False, dtype, offset=o, scale=s)
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
    decode_both(c, src, off, size, [a.nbytes for a in reads], opts, False, torch.float32, offset=o, scale=s,
                after_typed=lambda: paths.append(c.decode_paths()))
    assert paths[0][0] == n and paths[0][2] == n, paths
    c.close()


def test_fast5_chunks():
    c = codec()
    idx = json.load(open(os.path.join(GOLDEN, "fast5_chunks.json")))
    blob = np.fromfile(os.path.join(GOLDEN, "fast5_chunks.bin"), np.uint8)
    chunks = [blob[e["chunk_offset"] : e["chunk_offset"] + e["chunk_size"]] for e in idx]
    src, off, size = arena(c, chunks, 16)
    opts = c.options(True, 2, 1, 0)
    rng = np.random.default_rng(51)
    o, s = calibration(rng, len(idx), overflow=False)
    caps = [2 * e["samples"] for e in idx]
    for dtype in DTYPES:
        rt = decode_both(c, src, off, size, caps, opts, True, dtype, offset=o, scale=s)
        assert [int(r) for r in rt] == [e["samples"] * ELEM[key(dtype)] for e in idx]
    # (and the int16 samples those were held to are the golden ones)
    dev = c.device
    roff, rtot = batch.layout(caps, 64)
    raw = torch.zeros(rtot, dtype=torch.uint8, device=dev)
    res = torch.zeros(len(idx), dtype=torch.int32, device=dev)
    c.decompress(src, off, size, raw, roff.to(dev), i32(caps).to(dev), res, opts, sized=True)
    h = raw.cpu().numpy()
    for i, e in enumerate(idx):
        o_ = int(roff[i])
        assert hashlib.sha256(h[o_ : o_ + caps[i]].tobytes()).hexdigest() == e["raw_sha256"]


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
        decode_both(c, src, off, size, [2 * x for x in lens], opts, False, dtype, offset=o, scale=s)


# ---- 3. verdicts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
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
                p = offs[i] + int(rng.integers(4, sizes[i]))
                h[p] ^= 0xFF
            elif kind == 1 and sizes[i] > 2:
                sizes[i] = int(rng.integers(1, sizes[i]))
            elif sizes[i] > 8:
                h[offs[i] + sizes[i] - 1] ^= 0x01
        dsrc = torch.from_numpy(h).to(c.device)
        caps = [a.nbytes for a in reads]
        if sized:
            for i in range(1, n, 7):   # a capacity too small for the header's size
                caps[i] = max(0, caps[i] - 2)
        decode_both(c, dsrc, off, i32(sizes).to(c.device), caps, opts, sized, dtype, offset=np.full(n, 3.0, np.float32),
                    scale=np.full(n, 0.5, np.float32))


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
            for dtype in (torch.float32, torch.bfloat16):
                decode_both(c, src, off, size, caps, opts, sized, dtype, signed=zz)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_slot_alignment(dtype):
    """Offsets or capacities that are not multiples of E: VBZ_DESTINATION_SIZE_ERROR, the slot untouched; E-aligned slots off the 16-byte
    grid (every skew of E bytes) decode on the scalar store path."""
    c = codec()
    E = ELEM[key(dtype)]
    lens = [3, 8, 2047, 4096, 70001, 100000]
    reads = [O.synth_signal(18, i, x) for i, x in enumerate(lens)]
    opts = c.options(True, 2, 1, 1)
    src, off, size = compress(c, reads, opts)
    caps16 = [a.nbytes for a in reads]
    rng = np.random.default_rng(81)
    o, s = calibration(rng, len(reads), overflow=False)
    for skew in range(0, 16 // E):
        decode_both(c, src, off, size, caps16, opts, False, dtype, offset=o, scale=s, skew=skew)
    # misaligned offsets (read 1, 4) and capacities (read 2, 5), for every output type
    tcap = [x // 2 * E for x in caps16]
    toff = [k * (4 * 100000 + 256) for k in range(len(reads))]
    toff[1] += 1
    toff[4] += E - 1
    tcap[2] += 1
    tcap[5] -= 1
    decode_both(c, src, off, size, caps16, opts, False, dtype, offset=o, scale=s, typed_cap=tcap, typed_off=toff,
                expect={1: E_DEST, 2: E_DEST, 4: E_DEST, 5: E_DEST})


# ---- 4. host refusals ------------------------------------------------------------------------------------------------------
def test_host_refusals():
    c = codec()
    dev = c.device
    L = c.L
    reads = [O.synth_signal(19, 0, 1000)]
    opts = c.options(True, 2, 1, 1)
    src, off, size = compress(c, reads, opts)
    dst = torch.zeros(4096, dtype=torch.uint8, device=dev)
    doff = torch.zeros(1, dtype=torch.int64, device=dev)
    dcap = i32([4000]).to(dev)
    res = torch.full((1,), -8, dtype=torch.int32, device=dev)
    b = c._batch(src, off, size, dst, doff, dcap, res)

    def call(o=opts, f="ok", bt=b):
        if f == "ok":
            f = _lib.GpuSignalFormat()
            f.out_type, f.is_signed = _lib.VBZ_GPU_SIGNAL_F32, 1
        return L.vbz_gpu_decompress_signal_batch(c.ctx, ctypes.byref(bt) if bt is not None else None, ctypes.byref(o) if o is not None else None, 0,
                                                 ctypes.byref(f) if f is not None else None)

    def fmt(t, sg):
        f = _lib.GpuSignalFormat()
        f.out_type, f.is_signed = t, sg
        return f

    for isz, ver in ((1, 1), (4, 1), (0, 1), (2, 2)):
        assert call(o=c.options(True, isz, 1, ver)) == -2, (isz, ver)
    assert call(o=None) == -2
    assert call(f=None) == -2
    for t, sg in ((0, 1), (4, 1), (1, 2), (3, 0xFFFFFFFF)):
        assert call(f=fmt(t, sg)) == -2, (t, sg)
    bad = c._batch(src, off, size, dst, doff, dcap, res)
    bad.src_off = None
    assert call(bt=bad) == -2
    big = c._batch(src, off, size, dst, doff, dcap, res)
    big.dst_bytes = (1 << 46) + 1
    assert call(bt=big) == -2
    torch.cuda.synchronize()
    assert int(res[0]) == -8, "nothing was launched"
    assert L.vbz_gpu_decompress_signal_batch(c.ctx, None, ctypes.byref(opts), 0, ctypes.byref(fmt(1, 1))) == -1
    assert call() == 0
    torch.cuda.synchronize()
    assert int(res[0]) == 4000


# ---- 5. Python round trip --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_packed_round_trip(dtype):
    c = codec()
    rng = np.random.default_rng(91)
    lens = [0, 1, 17] + _ragged(rng, 200, 100, 60000) + [300_000]
    reads = [O.synth_signal(20, i, x) for i, x in enumerate(lens)]
    opts = c.options(True, 2, 1, 1)
    comp, coff, res = compress(c, reads, opts, sized=True)
    caps = [c.L.vbz_max_compressed_size(int(a.nbytes), ctypes.byref(opts)) for a in reads]
    packed, poff, psize = c.pack(comp, coff, i32(caps).to(c.device), res, align=16)
    o, s = calibration(rng, len(reads), overflow=False)
    out, out_off, samples, result = c.decompress_packed_signal(packed, poff, psize, opts, dtype=dtype, offset=torch.from_numpy(o).to(c.device),
                                                               scale=torch.from_numpy(s).to(c.device))
    torch.cuda.synchronize()
    assert out.dtype == dtype
    E = ELEM[key(dtype)]
    oo, ss, rr = out_off.cpu().tolist(), samples.cpu().tolist(), u32(result)
    h = out.view(torch.int16 if E == 2 else torch.int32).cpu().numpy()
    for i, a in enumerate(reads):
        assert ss[i] == a.size and int(rr[i]) == a.size * E, (i, ss[i], int(rr[i]))
        assert (oo[i] * E) % 16 == 0
        ref = typed_bits(a, o[i], s[i], key(dtype))
        assert np.array_equal(h[oo[i] : oo[i] + a.size].view(ref.dtype), ref), i
