"""Dense arenas on the MI355X (include/vbz_gpu.h: vbz_gpu_pack_batch, vbz_gpu_decompressed_size_batch; batch.GpuCodec.pack,
decompressed_sizes, decompress_packed): every arena byte against numpy, untrusted result tables, round trips through the codec."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import oracle_lib as O
from typed_support import codec, i32, u32
from vbz_compression_amd import _lib, batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
U32 = 0xFFFFFFFF

def ref_pack(dst, dst_bytes, dst_off, dst_cap, result, align):
    """numpy statement of vbz_gpu_pack_batch: (packed_off [n + 1], packed_size [n], arena bytes)"""
    n = len(result)
    size = np.zeros(n, np.uint64)
    take = np.zeros(n, np.uint64)
    for i in range(n):
        r = int(result[i])
        if r >= _lib.VBZ_DEVICE_ERROR:
            size[i] = r
        elif r > dst_cap[i] or dst_off[i] > dst_bytes or dst_cap[i] > dst_bytes - dst_off[i]:
            size[i] = _lib.VBZ_INPUT_SIZE_ERROR
        else:
            size[i] = r
            take[i] = (r + align - 1) // align * align
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(take)
    arena = np.zeros(int(off[n]), np.uint8)
    for i in range(n):
        if take[i]:
            arena[int(off[i]) : int(off[i]) + int(size[i])] = dst[int(dst_off[i]) : int(dst_off[i]) + int(size[i])]
    return off, size, arena


def fabricate(sizes, skew=True, seed=0, slack=64):
    """slots of random bytes: read i's slot at an offset with skew i % 16 and a capacity a little above its size"""
    rng = np.random.default_rng(seed)
    sizes = [int(s) for s in sizes]
    caps = [s + int(rng.integers(0, 40)) for s in sizes]
    off, pos = [], 0
    for i, c in enumerate(caps):
        pos = (pos + 15) // 16 * 16 + ((i % 16) if skew else 0)
        off.append(pos)
        pos += c
    dst = rng.integers(0, 256, pos + slack, dtype=np.uint8)
    return dst, np.array(off, np.uint64), np.array(caps, np.uint64), np.array(sizes, np.uint64)


def run_pack(dst, dst_bytes, dst_off, dst_cap, result, align, packed_cap=None, canary=None, null_packed=False):
    """the C call through ctypes; returns (rc, packed_off, packed_size, arena bytes or None)"""
    c = codec()
    dev = c.device
    d = torch.from_numpy(dst).to(dev)
    t_off = torch.tensor(dst_off.astype(np.int64)).to(dev)
    t_cap = i32(dst_cap).to(dev)
    t_res = i32(result).to(dev)
    n = len(result)
    poff = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    psize = torch.zeros(n, dtype=torch.int32, device=dev)
    b = _lib.GpuBatch()
    b.n_reads = n
    b.dst = d.data_ptr()
    b.dst_off = t_off.data_ptr()
    b.dst_cap = t_cap.data_ptr()
    b.dst_bytes = dst_bytes
    b.result = t_res.data_ptr()
    packed = None
    if not null_packed:
        cap = packed_cap if packed_cap is not None else int(ref_pack(dst, dst_bytes, dst_off, dst_cap, result, align)[0][n])
        fill = 0xA5 if canary is None else canary
        packed = torch.full((cap + 64,), fill, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rc = c.L.vbz_gpu_pack_batch(c.ctx, ctypes.byref(b), align, packed.data_ptr() if packed is not None else None,
                                cap if packed is not None else 0, poff.data_ptr(), psize.data_ptr())
    c.synchronize()
    return rc, poff.cpu().numpy().astype(np.uint64), u32(psize), (packed.cpu().numpy() if packed is not None else None)


def check_pack(dst, dst_off, dst_cap, result, align):
    ro, rs, ra = ref_pack(dst, len(dst), dst_off, dst_cap, result, align)
    rc, po, ps, arena = run_pack(dst, len(dst), dst_off, dst_cap, result, align)
    assert rc == 0
    assert np.array_equal(po, ro), align
    assert np.array_equal(ps, rs), align
    total = int(ro[-1])
    assert np.array_equal(arena[:total], ra), align
    assert (arena[total:] == 0xA5).all(), "nothing behind the total"
    return arena[:total]


@pytest.mark.parametrize("align", [1, 2, 16, 64, 4096])
def test_pack_every_skew_and_size(align):
    rng = np.random.default_rng(align)
    sizes = [0] + list(range(1, 32)) + rng.integers(38000, 42000, 48).tolist() + list(range(31, 0, -1))
    dst, off, cap, res = fabricate(sizes, seed=align)
    first = check_pack(dst, off, cap, res, align)
    again = check_pack(dst, off, cap, res, align)
    assert np.array_equal(first, again), "two calls, identical arenas"


@pytest.mark.parametrize("align", [1, 16])
def test_pack_one_40mb_read(align):
    sizes = [3, 40 << 20, 5]
    dst, off, cap, res = fabricate(sizes, seed=7)
    check_pack(dst, off, cap, res, align)


@pytest.mark.parametrize("align", [1, 16])
def test_pack_million_tiny_reads(align):
    n = 1 << 20
    rng = np.random.default_rng(11 + align)
    sizes = rng.integers(1, 65, n).astype(np.uint64)
    cap = sizes + rng.integers(0, 4, n).astype(np.uint64)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(cap)[:-1]
    off += np.arange(n, dtype=np.uint64) % 3   # slots shifted by 0-2 bytes, overlapping neighbours' slack: pack reads only result[i] bytes
    dst = rng.integers(0, 256, int(off[-1] + cap[-1]) + 64, dtype=np.uint8)
    ro, rs = np.zeros(n + 1, np.uint64), sizes.copy()
    take = (sizes + align - 1) // align * align
    ro[1:] = np.cumsum(take)
    rc, po, ps, arena = run_pack(dst, len(dst), off, cap, sizes, align, packed_cap=int(ro[n]))
    assert rc == 0
    assert np.array_equal(po, ro) and np.array_equal(ps, rs)
    # every arena byte: gather the expected bytes with numpy
    want = np.zeros(int(ro[n]), np.uint8)
    idx = np.repeat(np.arange(n), sizes.astype(np.int64))
    within = np.arange(int(sizes.sum()), dtype=np.int64) - np.repeat(np.cumsum(sizes.astype(np.int64)) - sizes.astype(np.int64), sizes.astype(np.int64))
    want[ro[idx].astype(np.int64) + within] = dst[off[idx].astype(np.int64) + within]
    assert np.array_equal(arena[: int(ro[n])], want)
    assert (arena[int(ro[n]) :] == 0xA5).all()


def test_pack_untrusted_results():
    sizes = [100, 200, 300, 400, 500, 600, 700, 800, 900, 1000, 50, 60]
    dst, off, cap, res = fabricate(sizes, seed=3, slack=4096)
    declared = int(off[-1] + cap[-1])   # the last slot ends the declared arena; 4 KB of canary behind it
    dst[declared:] = 0xEE
    res = res.copy()
    res[1] = _lib.VBZ_DEVICE_ERROR
    res[2] = _lib.VBZ_ZSTD_ERROR
    res[3] = _lib.VBZ_DESTINATION_SIZE_ERROR
    res[4] = cap[4] + 1                  # a count beyond its slot
    off = off.copy()
    off[5] = declared + 1000             # a slot beyond dst_bytes (inside the allocation: canary bytes, never read)
    off[6] = declared - 100              # a slot that runs past dst_bytes
    ro, rs, ra = ref_pack(dst, declared, off, cap, res, 16)
    assert list(rs[1:7]) == [_lib.VBZ_DEVICE_ERROR, _lib.VBZ_ZSTD_ERROR, _lib.VBZ_DESTINATION_SIZE_ERROR] + [_lib.VBZ_INPUT_SIZE_ERROR] * 3
    rc, po, ps, arena = run_pack(dst, declared, off, cap, res, 16)
    assert rc == 0 and np.array_equal(po, ro) and np.array_equal(ps, rs)
    assert np.array_equal(arena[: int(ro[-1])], ra)
    total = int(ro[-1])
    # an arena one byte short: untouched, the tables still complete
    rc, po, ps, arena = run_pack(dst, declared, off, cap, res, 16, packed_cap=total - 1, canary=0x3C)
    assert rc == 0 and int(po[-1]) == total and np.array_equal(po, ro) and np.array_equal(ps, rs)
    assert (arena == 0x3C).all()
    # no arena: the tables alone
    rc, po, ps, arena = run_pack(dst, declared, off, cap, res, 16, null_packed=True)
    assert rc == 0 and arena is None and np.array_equal(po, ro) and np.array_equal(ps, rs)


def test_pack_argument_checks():
    c = codec()
    dev = c.device
    n = 4
    d = torch.zeros(4096, dtype=torch.uint8, device=dev)
    t_off = torch.arange(n, dtype=torch.int64, device=dev) * 1024
    t_cap = torch.full((n,), 1000, dtype=torch.int32, device=dev)
    t_res = torch.full((n,), 10, dtype=torch.int32, device=dev)
    poff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    psize = torch.zeros(n, dtype=torch.int32, device=dev)
    packed = torch.zeros(4096, dtype=torch.uint8, device=dev)

    def call(align=16, **kw):
        b = _lib.GpuBatch()
        b.n_reads = n
        b.dst, b.dst_off, b.dst_cap, b.dst_bytes, b.result = d.data_ptr(), t_off.data_ptr(), t_cap.data_ptr(), 4096, t_res.data_ptr()
        for k, v in kw.items():
            setattr(b, k, v)
        return c.L.vbz_gpu_pack_batch(c.ctx, ctypes.byref(b), align, packed.data_ptr(), packed.numel(), poff.data_ptr(), psize.data_ptr())

    assert call(3) == -2
    assert call(8192) == -2
    assert call(0) == -2
    assert call(result=None) == -2
    assert call(dst_off=None) == -2
    assert call(dst_bytes=(1 << 46) + 1) == -2
    assert call() == 0   # src fields all NULL
    c.synchronize()
    assert poff.cpu().tolist() == [0, 16, 32, 48, 64]
    bad = _lib.GpuBatch()
    bad.n_reads, bad.dst, bad.dst_off, bad.dst_cap, bad.dst_bytes, bad.result = n, d.data_ptr(), t_off.data_ptr(), t_cap.data_ptr(), 4096, t_res.data_ptr()
    assert c.L.vbz_gpu_pack_batch(c.ctx, ctypes.byref(bad), 16, d.data_ptr() + 100, 1000, poff.data_ptr(), psize.data_ptr()) == -2, "overlap"


# ---- round trips through the codec -------------------------------------------------------------------------------------------
def _compress_reads(reads, opts, sized):
    c = codec()
    dev = c.device
    sizes = [int(a.nbytes) for a in reads]
    off, total = batch.layout(sizes, 64)
    arena = np.zeros(total, np.uint8)
    for a, o in zip(reads, off.tolist()):
        arena[o : o + a.nbytes] = np.frombuffer(a.tobytes(), np.uint8)
    caps = [c.L.vbz_max_compressed_size(s, ctypes.byref(opts)) for s in sizes]
    doff, dtotal = batch.layout(caps, 64)
    src = torch.from_numpy(arena).to(dev)
    dst = torch.empty(dtotal, dtype=torch.uint8, device=dev)
    dst_off, dst_cap = doff.to(dev), i32(caps).to(dev)
    res = torch.zeros(len(reads), dtype=torch.int32, device=dev)
    c.compress(src, off.to(dev), i32(sizes).to(dev), dst, dst_off, dst_cap, res, opts, sized=sized)
    return dst, dst_off, dst_cap, res


def _round_trip(reads, opts, sized):
    c = codec()
    dev = c.device
    dst, dst_off, dst_cap, res = _compress_reads(reads, opts, sized)
    packed, poff, psize = c.pack(dst, dst_off, dst_cap, res, align=16)
    torch.cuda.synchronize()
    assert np.array_equal(u32(psize), u32(res))
    if sized:
        raw, raw_off, raw_size, result = c.decompress_packed(packed, poff, psize, opts)
    else:
        n = len(reads)
        sizes = [int(a.nbytes) for a in reads]
        ro, rtotal = batch.layout(sizes, 16)
        raw = torch.empty(rtotal, dtype=torch.uint8, device=dev)
        raw_off = ro.to(dev)
        result = torch.zeros(n, dtype=torch.int32, device=dev)
        c.decompress(packed, poff[:n], psize, raw, raw_off, i32(sizes).to(dev), result, opts)
    torch.cuda.synchronize()
    h = raw.cpu().numpy()
    ro = raw_off.cpu().tolist()
    for i, a in enumerate(reads):
        assert int(result[i]) == a.nbytes, (i, int(result[i]) & U32)
        assert h[ro[i] : ro[i] + a.nbytes].tobytes() == a.tobytes(), i
    return c


@pytest.mark.parametrize("sized", [False, True])
def test_round_trip_ragged_with_large_reads(sized):
    rng = np.random.default_rng(5 + sized)
    lens = [0, 1, 3, 17, 1000] + rng.integers(100, 120000, 200).tolist() + [300_000, 600_000]   # 1.2 MB reads: the large-read path
    reads = [O.synth_signal(5, i, n) for i, n in enumerate(lens)]
    _round_trip(reads, codec().options(True, 2, 1, 1), sized)


def test_round_trip_with_checksums():
    c = codec()
    c.set_checksum(True)
    try:
        lens = [5, 999, 40000, 90000, 110000] * 20
        reads = [O.synth_signal(6, i, n) for i, n in enumerate(lens)]
        _round_trip(reads, c.options(True, 2, 1, 1), True)
    finally:
        c.set_checksum(False)


def test_packed_align16_arena_on_the_batched_decoder():
    c = codec()
    dev = c.device
    n = 3000
    opts = c.options(True, 2, 1, 1)
    lens = c.synth_lengths(17, 0, n)
    sizes = lens.to(torch.int64) * 2
    off, total = batch.layout(sizes.cpu(), 64)
    src = torch.zeros(total, dtype=torch.uint8, device=dev)
    c.synth_signal(17, 0, src, off.to(dev), lens)
    caps = torch.tensor([c.L.vbz_max_compressed_size(int(s), ctypes.byref(opts)) for s in sizes.cpu().tolist()], dtype=torch.int64)
    coff, ctotal = batch.layout(caps, 64)
    comp = torch.empty(ctotal, dtype=torch.uint8, device=dev)
    res = torch.zeros(n, dtype=torch.int32, device=dev)
    c.compress(src, off.to(dev), sizes.to(torch.int32).to(dev), comp, coff.to(dev), caps.to(torch.int32).to(dev), res, opts)
    packed, poff, psize = c.pack(comp, coff.to(dev), caps.to(torch.int32).to(dev), res, align=16)
    back = torch.zeros(total, dtype=torch.uint8, device=dev)
    result = torch.zeros(n, dtype=torch.int32, device=dev)
    c.decompress(packed, poff[:n], psize, back, off.to(dev), sizes.to(torch.int32).to(dev), result, opts)
    frames, batched, walked = c.decode_paths()
    assert frames == n and batched == n, (frames, batched, walked)
    torch.cuda.synchronize()
    assert torch.equal(result.to(torch.int64), sizes.to(dev))
    assert torch.equal(back, src)


def test_packed_fast5_chunks_decode_to_golden():
    c = codec()
    dev = c.device
    idx = json.load(open(os.path.join(GOLDEN, "fast5_chunks.json")))
    blob = np.fromfile(os.path.join(GOLDEN, "fast5_chunks.bin"), np.uint8)
    sizes = [e["chunk_size"] for e in idx]
    # the chunks in slots of their own (skewed, with room to spare), packed, decoded from the packed arena
    stride = (max(sizes) + 64 + 4095) // 4096 * 4096
    slot_off = np.array([i * stride + 3 * i for i in range(len(idx))], np.uint64)
    dst = np.zeros(len(idx) * stride + 64, np.uint8)
    for e, o in zip(idx, slot_off):
        dst[int(o) : int(o) + e["chunk_size"]] = blob[e["chunk_offset"] : e["chunk_offset"] + e["chunk_size"]]
    d = torch.from_numpy(dst).to(dev)
    packed, poff, psize = c.pack(d, torch.tensor(slot_off.astype(np.int64)).to(dev), i32([x + 40 for x in sizes]).to(dev),
                                 i32(sizes).to(dev), align=16)
    raw, raw_off, raw_size, result = c.decompress_packed(packed, poff, psize, c.options(True, 2, 1, 0))
    torch.cuda.synchronize()
    h = raw.cpu().numpy()
    ro = raw_off.cpu().tolist()
    for i, e in enumerate(idx):
        assert int(raw_size[i]) == 2 * e["samples"] and int(result[i]) == 2 * e["samples"]
        assert hashlib.sha256(h[ro[i] : ro[i] + 2 * e["samples"]].tobytes()).hexdigest() == e["raw_sha256"], e["read"]


# ---- sized layout --------------------------------------------------------------------------------------------------------------
def test_decompressed_sizes_match_the_single_buffer_call():
    c = codec()
    dev = c.device
    L = c.L
    opts = c.options(True, 2, 1, 1)
    reads = [O.synth_signal(8, i, n) for i, n in enumerate([0, 1, 2, 100, 5000, 70000])]
    bufs = [np.frombuffer(O.compress(a, O.options(True, 2, 1, 1), sized=True).tobytes(), np.uint8) for a in reads]
    bufs += [np.zeros(0, np.uint8), np.array([7], np.uint8), np.array([1, 2], np.uint8), np.array([1, 2, 3], np.uint8),
             np.array([0xFF, 0xFF, 0xFF, 0xFF, 0], np.uint8), np.array([5, 0, 0, 0], np.uint8)]
    sizes = [b.nbytes for b in bufs]
    off, total = batch.layout(sizes, 16)
    off = off.numpy() + 5   # unaligned headers
    arena = np.zeros(total + 5 + 64, np.uint8)
    for b, o in zip(bufs, off):
        arena[o : o + b.nbytes] = b
    want = [L.vbz_decompressed_size(b.ctypes.data if b.nbytes else None, b.nbytes, ctypes.byref(opts)) for b in bufs]
    # one buffer outside the declared arena
    off = np.append(off, total + 1000)
    sizes.append(8)
    want.append(_lib.VBZ_INPUT_SIZE_ERROR)
    src = torch.from_numpy(arena).to(dev)
    t_off, t_size = torch.tensor(off.astype(np.int64)).to(dev), i32(sizes).to(dev)
    for align in (1, 16, 64):
        raw_size, raw_off = c.decompressed_sizes(src, t_off, t_size, opts, align)
        torch.cuda.synchronize()
        got = u32(raw_size)
        assert got.tolist() == want, align
        take = [0 if w >= _lib.VBZ_DEVICE_ERROR else (w + align - 1) // align * align for w in want]
        assert raw_off.cpu().tolist() == np.concatenate([[0], np.cumsum(take)]).tolist()
    # bad options and alignments are refused before anything runs
    b = _lib.GpuBatch()
    b.n_reads, b.src, b.src_off, b.src_size, b.src_bytes = len(sizes), src.data_ptr(), t_off.data_ptr(), t_size.data_ptr(), src.numel()
    rs = torch.zeros(len(sizes), dtype=torch.int32, device=dev)
    ro = torch.zeros(len(sizes) + 1, dtype=torch.int64, device=dev)
    bad = _lib.CompressionOptions(True, 3, 1, 1)
    assert L.vbz_gpu_decompressed_size_batch(c.ctx, ctypes.byref(b), ctypes.byref(bad), 16, rs.data_ptr(), ro.data_ptr()) == -2
    assert L.vbz_gpu_decompressed_size_batch(c.ctx, ctypes.byref(b), ctypes.byref(opts), 24, rs.data_ptr(), ro.data_ptr()) == -2
    assert L.vbz_gpu_decompressed_size_batch(c.ctx, ctypes.byref(b), ctypes.byref(opts), 16, None, ro.data_ptr()) == -2
    b.dst_off = None   # the dst side is not looked at
    assert L.vbz_gpu_decompressed_size_batch(c.ctx, ctypes.byref(b), ctypes.byref(opts), 16, rs.data_ptr(), ro.data_ptr()) == 0
    c.synchronize()


def test_decompress_packed_verdicts_match_the_single_buffer_call():
    c = codec()
    dev = c.device
    L = c.L
    opts = c.options(True, 2, 1, 1)
    reads = [O.synth_signal(9, i, n) for i, n in enumerate([0, 10, 3000, 40000])]
    bufs = [np.frombuffer(O.compress(a, O.options(True, 2, 1, 1), sized=True).tobytes(), np.uint8) for a in reads]
    bufs += [np.zeros(0, np.uint8), np.array([9, 9], np.uint8), np.array([1, 2, 3], np.uint8), np.array([8, 0, 0, 0, 1, 2, 3], np.uint8)]
    bad = bufs[2].copy()
    bad[20] ^= 0x5A
    bufs.append(bad)
    sizes = [b.nbytes for b in bufs]
    off, total = batch.layout(sizes, 16)
    arena = np.zeros(total + 64, np.uint8)
    for b, o in zip(bufs, off.tolist()):
        arena[o : o + b.nbytes] = b
    want = []
    for b in bufs:
        cap = L.vbz_decompressed_size(b.ctypes.data if b.nbytes else None, b.nbytes, ctypes.byref(opts))
        cap = 0 if cap >= _lib.VBZ_DEVICE_ERROR else cap
        out = np.zeros(cap + 16, np.uint8)
        want.append(L.vbz_decompress_sized(b.ctypes.data if b.nbytes else None, b.nbytes, out.ctypes.data, cap, ctypes.byref(opts)))
    packed = torch.from_numpy(arena).to(dev)
    poff = torch.cat([off, torch.tensor([total])]).to(dev)
    raw, raw_off, raw_size, result = c.decompress_packed(packed, poff, i32(sizes).to(dev), opts)
    torch.cuda.synchronize()
    assert u32(result).tolist() == want
    h = raw.cpu().numpy()
    ro = raw_off.cpu().tolist()
    for i, a in enumerate(reads):
        assert h[ro[i] : ro[i] + a.nbytes].tobytes() == a.tobytes()
