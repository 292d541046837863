"""POD5 signal rows on the MI355X (include/vbz_gpu.h: VBZ_GPU_VERSION_POD5).  The svb16 stage is held byte for byte to tests/pod5_ref.py
in both directions; rows libzstd wrote (as pod5 does) decode bit-exact in every output and call shape of the int16 call; rows the library
writes decode with libzstd + pod5_ref; verdicts row by row; host refusals; the read layout of several rows; the compression ratio."""
import ctypes

import numpy as np
import pytest
import torch

import norm_ref as R
import oracle_lib as O
import pod5_ref as P
from signal_ref import chunk_rows, typed_bits
from typed_support import CANARY, ELEM, arena, codec, i32, key, pod5_compress, u32, walk_signal
from vbz_compression_amd import _lib, batch

pytestmark = pytest.mark.gpu

POD5 = _lib.VBZ_GPU_VERSION_POD5
E_ZSTD, E_DEST, E_STREAM = 0xFFFFFFFF, 0xFFFFFFFC, 0xFFFFFFFB
DTYPES = [torch.float32, torch.float16, torch.bfloat16]


def rows_of(seed, lens):
    """rows of several kinds: signal, full-range noise (two data bytes), the benchmark's synthetic signal"""
    rng = np.random.default_rng(seed)
    out = []
    for k, T in enumerate(lens):
        kind = k % 4
        if kind == 1:
            out.append(rng.integers(-32768, 32768, T).astype(np.int16))
        elif kind == 2:
            out.append(O.synth_signal(seed, k, T))
        else:
            out.append(walk_signal(rng, T))
    return out


def int16_layout(c, rows):
    dev = c.device
    off, total = batch.layout([2 * len(x) for x in rows], 16)
    return off.to(dev), i32([2 * len(x) for x in rows]).to(dev), total


def decode_int16(c, frames, rows, caps=None):
    src, off, size = arena(c, frames, 16)
    doff, dcap, total = int16_layout(c, rows)
    if caps is not None:   # (slots of the given capacities, apart)
        o, total = batch.layout([max(int(k), 2 * len(x)) + 16 for k, x in zip(caps, rows)], 16)
        doff, dcap = o.to(c.device), i32(caps).to(c.device)
    dst = torch.zeros(total + 64, dtype=torch.uint8, device=c.device)
    res = torch.full((len(rows),), -8, dtype=torch.int32, device=c.device)
    c.decompress(src, off, size, dst, doff, dcap, res, batch.pod5_options())
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    return u32(res), [host[o : o + 2 * len(x)].view(np.int16) for o, x in zip(doff.tolist(), rows)]


def check_outputs(c, frames, rows, typed=DTYPES, chunks=True, norms=True, seed=0):
    """every output of the decode against numpy: int16, calibrated F32 / F16 / BF16, chunks PAD / END (float16), MED_MAD / QUANTILE"""
    n = len(rows)
    dev = c.device
    res, got = decode_int16(c, frames, rows)
    assert all(int(r) == 2 * len(x) for r, x in zip(res, rows)), [(i, hex(int(r))) for i, r in enumerate(res) if int(r) != 2 * len(rows[i])][:4]
    for i, (g, x) in enumerate(zip(got, rows)):
        assert g.tobytes() == x.tobytes(), i
    src, off, size = arena(c, frames, 16)
    rng = np.random.default_rng(seed)
    o = rng.uniform(-600, 600, n).astype(np.float32)
    s = rng.uniform(0.01, 2.5, n).astype(np.float32)
    for dtype in typed:
        E = ELEM[key(dtype)]
        toff, tot = batch.layout([E * len(x) for x in rows], 16)
        dst = torch.zeros((tot + 64) // E, dtype=dtype, device=dev)
        tres = torch.full((n,), -8, dtype=torch.int32, device=dev)
        c.decompress_signal(src, off, size, dst, toff.to(dev), i32([E * len(x) for x in rows]).to(dev), tres, batch.pod5_options(),
                            offset=torch.from_numpy(o).to(dev), scale=torch.from_numpy(s).to(dev))
        torch.cuda.synchronize()
        assert (u32(tres) == np.array([E * len(x) for x in rows])).all(), dtype
        host = dst.view(torch.uint8).cpu().numpy()
        for i, x in enumerate(rows):
            want = typed_bits(x, o[i], s[i], key(dtype))
            assert host[toff[i] : toff[i] + E * len(x)].view(want.dtype).tobytes() == want.tobytes(), (dtype, i)
    if chunks:
        samples = i32([len(x) for x in rows]).to(dev)
        for mode, ea in (("pad", 1), ("end", 8)):
            L, S = 4000, 3600
            res = torch.full((n,), -8, dtype=torch.int32, device=dev)
            ch, first, _ = c.decompress_chunks(src, off, size, samples, res, batch.pod5_options(), L, S, mode=mode, end_align=ea, pad=-7.0,
                                               dtype=torch.float16, offset=torch.from_numpy(o).to(dev), scale=torch.from_numpy(s).to(dev))
            torch.cuda.synchronize()
            assert (u32(res) == np.array([2 * len(x) for x in rows])).all(), mode
            hc = ch.view(torch.int16).cpu().numpy().view(np.uint16)
            first = first.cpu().numpy()
            for i, x in enumerate(rows):
                st, want = chunk_rows(x, L, S, mode, ea, o[i], s[i], -7.0, "f16")
                assert first[i + 1] - first[i] == len(st), (mode, i)
                bad = np.argwhere(hc[first[i] : first[i + 1]] != want)
                assert bad.size == 0, (mode, i, bad[:4].tolist())
    if norms:
        doff, dcap, _ = int16_layout(c, rows)
        for p, nm in ((R.BONITO, batch.MED_MAD), (R.DORADO, batch.DORADO_QUANTILE)):
            res = torch.full((n,), -8, dtype=torch.int32, device=dev)
            ss = c.signal_norm(src, off, size, doff, dcap, res, batch.pod5_options(), nm)
            torch.cuda.synchronize()
            assert (u32(res) == np.array([2 * len(x) for x in rows])).all()
            ss = ss.cpu().numpy()
            for i, x in enumerate(rows):
                shift, scale = R.shift_scale(x, p)
                assert ss[i][0].view(np.uint32) == shift.view(np.uint32) and ss[i][1].view(np.uint32) == scale.view(np.uint32), (i, len(x))
            # ... and the normalised store is the calibrated store with those constants
            E = 2
            toff, tot = batch.layout([E * len(x) for x in rows], 16)
            dst = torch.zeros((tot + 64) // E, dtype=torch.float16, device=dev)
            c.decompress_signal(src, off, size, dst, toff.to(dev), i32([E * len(x) for x in rows]).to(dev), res, batch.pod5_options(), norm=nm)
            torch.cuda.synchronize()
            host = dst.view(torch.uint8).cpu().numpy()
            for i, x in enumerate(rows[:64]):
                _, _, so, sc = R.constants(*R.stats(x, p), p)
                want = typed_bits(x, so, sc, "f16")
                assert host[toff[i] : toff[i] + E * len(x)].view(np.uint16).tobytes() == want.tobytes(), i


# ---- the svb16 stage ------------------------------------------------------------------------------------------------------------
def stage(fn, bufs, caps):
    c = codec()
    dev = c.device
    src, off, size = arena(c, bufs, 16)
    doff, tot = batch.layout([int(x) + 32 for x in caps], 16)
    dst = torch.zeros(tot + 64, dtype=torch.uint8, device=dev)
    res = torch.full((len(bufs),), -8, dtype=torch.int32, device=dev)
    fn(c, src, off, size, dst, doff.to(dev), i32(caps).to(dev), res)
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    return [int(r) if _lib.is_error(int(r)) else host[o : o + int(r)].copy() for r, o in zip(u32(res), doff.tolist())]


def test_svb16_stage_bit_exact():
    lens = [0, 1, 2, 7, 8, 9, 15, 16, 17, 2047, 2048, 2049, 4095, 4096, 4097, 100_003, 5, 63, 64, 65] + list(range(300, 340))
    rows = rows_of(1, lens)
    rows.append(np.array([0, 1, -1, 300, 300], np.int16))
    rows.append(np.array([-32768, 32767], np.int16))
    enc = stage(lambda c, *a: c.svb_compress(*a, size=2, zigzag=True, version=POD5), rows, [P.svb16_max(len(x)) for x in rows])
    for i, (e, x) in enumerate(zip(enc, rows)):
        assert not isinstance(e, int), (i, hex(e))
        assert e.tobytes() == P.svb16_encode(x).tobytes(), i
    assert enc[-2].tobytes() == bytes.fromhex("08 00 02 03 5a 02 00") and enc[-1].tobytes() == bytes.fromhex("01 ff ff 01")
    streams = [P.svb16_encode(x) for x in rows]
    dec = stage(lambda c, *a: c.svb_decompress(*a, size=2, zigzag=True, version=POD5), streams, [2 * len(x) for x in rows])
    for i, (d, x) in enumerate(zip(dec, rows)):
        assert not isinstance(d, int), (i, hex(d))
        assert d.tobytes() == x.tobytes(), i
    # a slot below svb16_max(n) is refused
    small = stage(lambda c, *a: c.svb_compress(*a, size=2, zigzag=True, version=POD5), rows[15:16], [P.svb16_max(len(rows[15])) - 1])
    assert small == [E_DEST]


# ---- libzstd-written rows in every output and call shape --------------------------------------------------------------------
def test_libzstd_rows_small_batch():
    """a batch too small to fill the device: the large-read path (the svb16 stage one workgroup per row)"""
    rows = rows_of(2, [102_400, 100_003, 98_765, 4001, 0, 1, 17, 102_400])
    check_outputs(codec(), [P.compress_row(x) for x in rows], rows, seed=2)


def test_libzstd_rows_walked():
    c = codec()
    rng = np.random.default_rng(3)
    rows = rows_of(3, rng.integers(0, 6000, 2600).tolist())
    frames = [P.compress_row(x) for x in rows]
    check_outputs(c, frames, rows, typed=[torch.float16], chunks=False, norms=False, seed=3)
    decode_int16(c, frames, rows)
    n, batched, walked = c.decode_paths()
    assert n == len(rows) and walked > 0, (n, batched, walked)
    check_outputs(c, frames[:600], rows[:600], seed=3)


def test_libzstd_rows_split_halves():
    rng = np.random.default_rng(4)
    rows = rows_of(4, rng.integers(0, 1200, 16_400).tolist())
    check_outputs(codec(), [P.compress_row(x) for x in rows], rows, typed=[torch.bfloat16], chunks=False, norms=False, seed=4)


def test_libzstd_rows_routed():
    """rows of 512 KB and more among short ones: routed to the large-read path beside the rest"""
    rng = np.random.default_rng(5)
    lens = rng.integers(100, 5000, 300).tolist()
    lens[7] = 300_000
    lens[200] = 262_144
    rows = rows_of(5, lens)
    check_outputs(codec(), [P.compress_row(x) for x in rows], rows, seed=5)


def test_golden_rows_all_outputs():
    rows, _ = P.golden_rows()
    check_outputs(codec(), [P.compress_row(x) for x in rows], rows, seed=6)


# ---- rows the library writes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trailers,checksum", [(True, False), (False, False), (True, True)])
def test_library_rows_decode_with_libzstd(trailers, checksum):
    c = codec()
    c.set_trailers(trailers)
    c.set_checksum(checksum)
    try:
        rng = np.random.default_rng(7)
        for lens in ([102_400, 3, 0, 50_001, 700_000], rng.integers(0, 9000, 3000).tolist()):
            rows = rows_of(7, lens)
            frames = pod5_compress(c, rows)
            for i, (f, x) in enumerate(zip(frames, rows)):
                assert len(f) <= P.max_compressed_size(len(x)), i
                back = P.decompress_row(f, len(x))
                assert back is not None and back.tobytes() == x.tobytes(), i
            res, got = decode_int16(c, frames, rows)
            assert all(int(r) == 2 * len(x) for r, x in zip(res, rows))
            assert all(g.tobytes() == x.tobytes() for g, x in zip(got, rows))
    finally:
        c.set_trailers(True)
        c.set_checksum(False)


def test_canonical_bytes():
    c = codec()
    c.set_canonical(True)
    try:
        rng = np.random.default_rng(8)
        rows = rows_of(8, rng.integers(2000, 20_000, 4096).tolist())
        whole = pod5_compress(c, rows)
        for i in (0, 1, 2, 3, 1000, 4095):
            assert pod5_compress(c, [rows[i]])[0].tobytes() == whole[i].tobytes(), i
    finally:
        c.set_canonical(False)


# ---- verdicts ---------------------------------------------------------------------------------------------------------------------
def test_verdicts_row_by_row():
    c = codec()
    rows = rows_of(9, [5000, 5000, 5000, 5000, 5000, 5000, 20, 5000])
    good = [P.compress_row(x) for x in rows]
    frames, want = list(good), [2 * len(x) for x in rows]
    frames[0] = good[0][: len(good[0]) // 2]                                      # truncated frame
    want[0] = E_ZSTD
    s = P.svb16_encode(rows[1])
    frames[1] = O.zstd_compress(s[:-1], 1)                                        # stream one byte short
    want[1] = E_STREAM
    frames[2] = O.zstd_compress(np.concatenate([P.svb16_encode(rows[2]), [0]]).astype(np.uint8), 1)   # one byte long
    want[2] = E_STREAM
    n3 = len(rows[3])
    frames[3] = O.zstd_compress(np.zeros(P.svb16_max(n3) + 1, np.uint8), 1)       # content above svb16_max(n)
    want[3] = E_ZSTD
    frames[4] = O.zstd_compress(np.zeros(P.svb16_max(n3), np.uint8), 1)           # at svb16_max(n), but the wrong length
    want[4] = E_STREAM
    frames[6] = O.zstd_compress(np.ones(3 * 20 + 40, np.uint8), 1)                # a short row, far too much content
    want[6] = E_ZSTD
    res, got = decode_int16(c, frames, rows)
    assert [int(r) for r in res] == want, [hex(int(r)) for r in res]
    for i in (5, 7):
        assert got[i].tobytes() == rows[i].tobytes()
    # the same frames through the chunk and signal calls: the same verdicts
    src, off, size = arena(c, frames, 16)
    dst = torch.zeros(8 * 5000 * 4 + 4096, dtype=torch.float32, device=c.device)
    toff, _ = batch.layout([4 * len(x) for x in rows], 16)
    tres = torch.full((len(rows),), -8, dtype=torch.int32, device=c.device)
    c.decompress_signal(src, off, size, dst, toff.to(c.device), i32([4 * len(x) for x in rows]).to(c.device), tres, batch.pod5_options())
    torch.cuda.synchronize()
    assert [int(r) for r in u32(tres)] == [w if _lib.is_error(w) else 2 * w for w in want]


def test_dst_cap_mismatch_and_odd_caps():
    c = codec()
    rows = rows_of(10, [3000, 3000, 3000, 3000, 3000])
    frames = [P.compress_row(x) for x in rows]
    caps = [2 * 3000 + 2, 2 * 3000 - 2, 2 * 1000, 2 * 3000 + 1, 2 * 3000]
    res, _ = decode_int16(c, frames, rows, caps=caps)
    streams = [P.svb16_encode(x) for x in rows]
    for i in range(3):
        n = caps[i] // 2
        assert int(res[i]) == (E_ZSTD if len(streams[i]) > P.svb16_max(n) else E_STREAM), (i, hex(int(res[i])))
    assert int(res[4]) == 6000
    # an odd capacity: what the v0 int16 call gives for the same slot
    v0 = [O.compress(x, O.options(True, 2, 1, 0)) for x in rows]
    src, off, size = arena(c, v0, 16)
    doff, _, total = int16_layout(c, rows)
    dst = torch.zeros(total + 64, dtype=torch.uint8, device=c.device)
    r0 = torch.full((5,), -8, dtype=torch.int32, device=c.device)
    c.decompress(src, off, size, dst, doff, i32(caps).to(c.device), r0, c.options(True, 2, 1, 0))
    torch.cuda.synchronize()
    assert int(res[3]) == int(u32(r0)[3]) and _lib.is_error(int(res[3]))


def test_unaligned_typed_slots_keep_canaries():
    c = codec()
    dev = c.device
    rows = rows_of(11, [1000, 1001, 999, 1000])
    frames = [P.compress_row(x) for x in rows]
    src, off, size = arena(c, frames, 16)
    E = 4
    toff = [0, 4096 + 2, 8192, 12288 + 4]   # the second slot is not 4-byte aligned
    tcap = [E * len(x) for x in rows]
    tcap[2] += 2                            # the third capacity is not a multiple of 4
    arena_t = torch.full((16384 + 4096,), CANARY, dtype=torch.uint8, device=dev)
    res = torch.full((4,), -8, dtype=torch.int32, device=dev)
    c.decompress_signal(src, off, size, arena_t.view(torch.float32), torch.tensor(toff, dtype=torch.int64, device=dev), i32(tcap).to(dev), res,
                        batch.pod5_options())
    torch.cuda.synchronize()
    assert [int(r) for r in u32(res)] == [4000, E_DEST, E_DEST, 4000]
    host = arena_t.cpu().numpy()
    written = np.zeros(host.size, bool)
    for i in (0, 3):
        written[toff[i] : toff[i] + tcap[i]] = True
        assert host[toff[i] : toff[i] + tcap[i]].view(np.float32).tobytes() == rows[i].astype(np.float32).tobytes()
    assert (host[~written] == CANARY).all()


# ---- host refusals ----------------------------------------------------------------------------------------------------------------
def test_host_refusals():
    c = codec()
    L = c.L
    rows = rows_of(12, [100, 200])
    raw, off, size = arena(c, rows, 16)
    dst = torch.zeros(4096, dtype=torch.uint8, device=c.device)
    doff = torch.tensor([0, 1024], dtype=torch.int64, device=c.device)
    cap = i32([1024, 1024]).to(c.device)
    res = torch.zeros(2, dtype=torch.int32, device=c.device)
    b = c._batch(raw, off, size, dst, doff, cap, res)
    bad = [(True, 2, 1, POD5, 1), (True, 2, 0, POD5, 0), (False, 2, 1, POD5, 0), (True, 4, 1, POD5, 0), (True, 1, 1, POD5, 0), (True, 0, 1, POD5, 0)]
    for zz, isz, lvl, ver, sized in bad:
        o = _lib.CompressionOptions(zz, isz, lvl, ver)
        assert L.vbz_gpu_compress_batch(c.ctx, ctypes.byref(b), ctypes.byref(o), sized) == -2, (zz, isz, lvl, sized)
        assert L.vbz_gpu_decompress_batch(c.ctx, ctypes.byref(b), ctypes.byref(o), sized) == -2, (zz, isz, lvl, sized)
        f = _lib.GpuSignalFormat()
        f.out_type, f.is_signed = _lib.VBZ_GPU_SIGNAL_F32, 1
        assert L.vbz_gpu_decompress_signal_batch(c.ctx, ctypes.byref(b), ctypes.byref(o), sized, ctypes.byref(f)) == -2
    o = batch.pod5_options()
    sz = torch.zeros(2, dtype=torch.int32, device=c.device)
    roff = torch.zeros(3, dtype=torch.int64, device=c.device)
    assert L.vbz_gpu_decompressed_size_batch(c.ctx, ctypes.byref(b), ctypes.byref(o), 16, sz.data_ptr(), roff.data_ptr()) == -2
    assert L.vbz_gpu_svb_compress_batch(c.ctx, ctypes.byref(b), 2, 0, POD5) == -2
    assert L.vbz_gpu_svb_decompress_batch(c.ctx, ctypes.byref(b), 4, 1, POD5) == -2
    torch.cuda.synchronize()
    assert (res.cpu() == 0).all()   # (nothing was launched)


# ---- several rows of one read --------------------------------------------------------------------------------------------------------
def test_read_layout_contiguous_reads():
    c = codec()
    dev = c.device
    rng = np.random.default_rng(13)
    reads = [walk_signal(rng, 2 * P.ROW + 5000), walk_signal(rng, 777), walk_signal(rng, P.ROW + 3)]
    rows, first = [], []
    for x in reads:
        first.append(len(rows))
        rows += [x[s : s + P.ROW] for s in range(0, len(x), P.ROW)]
    assert first == [0, 3, 4]
    frames = [P.compress_row(x) for x in rows]
    src, off, size = arena(c, frames, 16)
    lay = batch.pod5_read_layout([len(x) for x in rows], first, device=dev)
    dst = torch.zeros(lay.total + 64, dtype=torch.uint8, device=dev)
    res = torch.full((len(rows),), -8, dtype=torch.int32, device=dev)
    c.decompress(src, off, size, dst, lay.dst_off, lay.dst_cap, res, batch.pod5_options())
    torch.cuda.synchronize()
    assert (u32(res) == np.array([2 * len(x) for x in rows])).all()
    for k, x in enumerate(reads):
        o, n = int(lay.read_off[k]), int(lay.read_len[k])
        assert n == len(x)
        assert torch.equal(dst[o : o + 2 * n].view(torch.int16).cpu(), torch.from_numpy(x))
    # calibrated: the read's offset and scale once per row
    lay4 = batch.pod5_read_layout([len(x) for x in rows], first, elem=4, device=dev)
    ro = np.array([10.0, -3.5, 0.25], np.float32)
    rs = np.array([0.5, 1.75, 2.0], np.float32)
    owner = np.repeat(np.arange(3), np.diff(first + [len(rows)]))
    out = torch.zeros((lay4.total + 64) // 4, dtype=torch.float32, device=dev)
    c.decompress_signal(src, off, size, out, lay4.dst_off, lay4.dst_cap, res, batch.pod5_options(),
                        offset=torch.from_numpy(ro[owner]).to(dev), scale=torch.from_numpy(rs[owner]).to(dev))
    torch.cuda.synchronize()
    for k, x in enumerate(reads):
        o = int(lay4.read_off[k]) // 4
        want = (x.astype(np.float32) + ro[k]) * rs[k]
        assert out[o : o + len(x)].cpu().numpy().view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), k


# ---- ratio ----------------------------------------------------------------------------------------------------------------------
def test_ratio_against_libzstd_level1():
    c = codec()
    golden, _ = P.golden_rows()
    lens = [O.synth_read_length(5, i) for i in range(256)]
    synth = [O.synth_signal(5, i, n) for i, n in enumerate(lens)]
    for rows in (golden, synth):
        ours = sum(len(f) for f in pod5_compress(c, rows))
        ref = sum(len(P.compress_row(x)) for x in rows)
        assert ours <= ref / 0.9, (ours, ref)
