"""The zstd content checksum (RFC 8878 3.1.1; include/vbz_gpu.h: vbz_gpu_set_checksum, vbz_gpu_xxh64_batch).  The authority is libzstd
1.4.8: its ZSTD_XXH64 for the hash, its checksum-writing compressor for frames of other writers, and ZSTD_decompress -- which verifies the
checksum, as the reference's vbz_decompress does through it -- for the verdicts."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gpu_util as G
import oracle_lib as O
import typed_support as S
from vbz_compression_amd import _lib, batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ZSTD = _lib.VBZ_ZSTD_ERROR


def _zstd():
    L = ctypes.CDLL("libzstd.so.1")
    L.ZSTD_XXH64.restype = ctypes.c_uint64
    L.ZSTD_XXH64.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64]
    L.ZSTD_createCCtx.restype = ctypes.c_void_p
    L.ZSTD_freeCCtx.argtypes = [ctypes.c_void_p]
    L.ZSTD_CCtx_setParameter.restype = ctypes.c_size_t
    L.ZSTD_CCtx_setParameter.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.ZSTD_compress2.restype = ctypes.c_size_t
    L.ZSTD_compress2.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    L.ZSTD_compressBound.restype = ctypes.c_size_t
    L.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
    L.ZSTD_isError.restype = ctypes.c_uint
    L.ZSTD_isError.argtypes = [ctypes.c_size_t]
    return L


Z = _zstd()


def xxh64(b):
    a = np.ascontiguousarray(np.frombuffer(bytes(b), np.uint8)) if not isinstance(b, np.ndarray) else np.ascontiguousarray(b).view(np.uint8)
    return Z.ZSTD_XXH64(a.ctypes.data if a.size else None, a.nbytes, 0)


def zstd_checksummed(data, level):
    """a zstd frame of `data` written by libzstd with Content_Checksum_flag (ZSTD_c_checksumFlag = 201, ZSTD_c_compressionLevel = 100)"""
    a = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    cap = Z.ZSTD_compressBound(a.nbytes)
    out = np.zeros(cap, np.uint8)
    cc = Z.ZSTD_createCCtx()
    try:
        assert not Z.ZSTD_isError(Z.ZSTD_CCtx_setParameter(cc, 100, level))
        assert not Z.ZSTD_isError(Z.ZSTD_CCtx_setParameter(cc, 201, 1))
        r = Z.ZSTD_compress2(cc, out.ctypes.data, cap, a.ctypes.data if a.size else None, a.nbytes)
        assert not Z.ZSTD_isError(r)
    finally:
        Z.ZSTD_freeCCtx(cc)
    f = out[:r].copy()
    assert f[4] & 4
    return f


def blocks_end(f, start=0):
    """(where the checksum of the zstd frame at f[start:] stands, the block types seen)"""
    f = bytes(f)
    fhd = f[start + 4]
    single, fcs_flag, did = (fhd >> 5) & 1, fhd >> 6, fhd & 3
    pos = start + 5 + (0 if single else 1) + (4 if did == 3 else did) + ((1 if single else 0) if fcs_flag == 0 else (1 << fcs_flag))
    types = []
    while True:
        bh = f[pos] | (f[pos + 1] << 8) | (f[pos + 2] << 16)
        bt, bs = (bh >> 1) & 3, bh >> 3
        types.append((bt, pos + 3, bs))
        pos += 3 + (1 if bt == 1 else bs)
        if bh & 1:
            return pos, types


def flip(f, at, bit=0):
    g = np.array(f, np.uint8, copy=True)
    g[at] ^= 1 << bit
    return g


def libzstd_ok(frame, cap):
    return O.zstd_decompress(frame, cap) is not None


@pytest.fixture
def fresh_codec():
    """a context of its own (per-context state such as the walk's knowledge of earlier calls does not leak between tests)"""
    old = S._codecs.get(())
    S._codecs[()] = batch.GpuCodec(0)   # (what codec() with no knob returns: gpu_util's stages run in it)
    try:
        yield S._codecs[()]
    finally:
        S._codecs.pop(()).close()
        if old is not None:
            S._codecs[()] = old


@pytest.fixture
def checksum_on(fresh_codec):
    """the writer on, in a context of its own (the shared context's modes are left as they were)"""
    fresh_codec.set_checksum(1)
    return fresh_codec


# ---- 1. the hash ------------------------------------------------------------------------------------------------------------------------
def _hash_batch(arena, offs, lens):
    c = G.codec()
    src = torch.from_numpy(arena).to(c.device)
    off = torch.tensor(offs, dtype=torch.int64, device=c.device)
    ln = torch.tensor(lens, dtype=torch.int64).to(torch.int32).to(c.device)
    out = torch.zeros(len(offs), dtype=torch.int64, device=c.device)
    c.xxh64(src, off, ln, out)
    torch.cuda.synchronize()
    return [int(x) & 0xFFFFFFFFFFFFFFFF for x in out.cpu().tolist()]


def test_xxh64_every_length_at_odd_offsets():
    rng = np.random.default_rng(1)
    lens = list(range(301))
    offs, pos = [], 1
    for n in lens:
        offs.append(pos)
        pos += n + 2 * (n % 5) + 1
        pos |= 1
    arena = rng.integers(0, 256, pos + 256, dtype=np.uint8)
    got = _hash_batch(arena, offs, lens)
    for o, n, h in zip(offs, lens, got):
        assert h == Z.ZSTD_XXH64(arena.ctypes.data + o, n, 0), (o, n)


def test_xxh64_65536_reads():
    rng = np.random.default_rng(2)
    lens = rng.integers(0, 3000, 65536).tolist()
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) + rng.integers(0, 4, 65536).cumsum()
    arena = rng.integers(0, 256, int(offs[-1]) + lens[-1] + 256, dtype=np.uint8)
    got = _hash_batch(arena, offs.tolist(), lens)
    for o, n, h in zip(offs.tolist(), lens, got):
        assert h == Z.ZSTD_XXH64(arena.ctypes.data + o, n, 0)


def test_xxh64_40_mb_buffer():
    rng = np.random.default_rng(3)
    n = 40_000_003
    arena = rng.integers(0, 256, n + 256, dtype=np.uint8)
    assert _hash_batch(arena, [3], [n])[0] == Z.ZSTD_XXH64(arena.ctypes.data + 3, n, 0)


# ---- 2. frames libzstd wrote with checksums ------------------------------------------------------------------------------------------------
def _reads(count, seed, lo=2000, hi=9000):
    rng = np.random.default_rng(seed)
    return [O.synth_signal(7, seed * 100000 + i, int(rng.integers(lo, hi))) for i in range(count)]


def _foreign(reads, level):
    return [zstd_checksummed(O.svb_compress(a, 2, True, 0), level) for a in reads]


def _damage(frames, every, rng):
    """one bit of the checksum of every `every`-th frame flipped: (frames, damaged indices)"""
    out, bad = [], set()
    for i, f in enumerate(frames):
        if i % every == 3:
            f = flip(f, len(f) - 1 - int(rng.integers(0, 4)), int(rng.integers(0, 8)))
            bad.add(i)
        out.append(f)
    return out, bad


def _check_verdicts(got, frames, reads, bad):
    for i, (g, a) in enumerate(zip(got, reads)):
        if i in bad:
            assert g == E_ZSTD, (i, g)
        else:
            assert not isinstance(g, int), (i, g)
            assert g.tobytes() == a.tobytes()


@pytest.mark.parametrize("level", [1, 3])
@pytest.mark.parametrize("count", [40, 4096, 16384])
def test_libzstd_checksummed_frames(level, count, fresh_codec):
    reads = _reads(count, level * 7 + count % 11, *((500, 3000) if count > 4096 else (2000, 9000)))
    frames = _foreign(reads, level)
    opts = _lib.CompressionOptions(True, 2, level, 0)
    caps = [a.nbytes for a in reads]
    got = G.decompress(frames, caps, opts)
    _check_verdicts(got, frames, reads, set())
    if count == 4096:
        n, b, w = G.codec().decode_paths()
        assert (n, w) == (count, count), "libzstd's frames with checksums are walked"
    rng = np.random.default_rng(count)
    damaged, bad = _damage(frames, 7, rng)
    for i in list(bad)[:50]:
        assert not libzstd_ok(damaged[i], caps[i] * 3)
    got = G.decompress(damaged, caps, opts)
    _check_verdicts(got, damaged, reads, bad)


@pytest.mark.parametrize("count", [40, 3000])
def test_damaged_raw_block_payload(count):
    """frames that parse but whose content is wrong: a bit flipped inside a raw block (incompressible bytes, integer_size 0)"""
    rng = np.random.default_rng(count + 5)
    bufs = [rng.integers(0, 256, int(rng.integers(100, 5000)), dtype=np.uint8) for _ in range(count)]
    frames = [zstd_checksummed(b, 1) for b in bufs]
    bad, damaged = set(), []
    for i, f in enumerate(frames):
        if i % 5 == 1:
            end, types = blocks_end(f)
            bt, at, bs = types[0]
            assert bt == 0 and bs > 10
            f = flip(f, at + int(rng.integers(0, bs)), int(rng.integers(0, 8)))
            assert not libzstd_ok(f, bufs[i].nbytes)
            bad.add(i)
        damaged.append(f)
    opts = _lib.CompressionOptions(False, 0, 1, 0)
    got = G.decompress(damaged, [b.nbytes for b in bufs], opts)
    _check_verdicts(got, damaged, bufs, bad)
    # the stage entry point: same verdicts
    got = G.zstd_decompress(damaged, [b.nbytes for b in bufs])
    _check_verdicts(got, damaged, bufs, bad)


def test_single_buffer_and_large_read():
    from vbz_compression_amd import vbz

    opts = _lib.CompressionOptions(True, 2, 1, 0)
    for a in (O.synth_signal(7, 1, 60000), O.synth_signal(7, 2, 4_000_000)):
        f = _foreign([a], 1)[0]
        back = vbz.decompress_raw(f, a.nbytes, opts)
        assert not isinstance(back, int) and back.tobytes() == a.tobytes()
        assert G.decompress([f], [a.nbytes], opts)[0].tobytes() == a.tobytes()
        bad = flip(f, len(f) - 2, 5)
        assert not libzstd_ok(bad, a.nbytes * 2)
        assert vbz.decompress_raw(bad, a.nbytes, opts) == E_ZSTD
        assert G.decompress([bad], [a.nbytes], opts)[0] == E_ZSTD
        end, types = blocks_end(f)
        raw = [t for t in types if t[0] == 0 and t[2] > 16]
        if raw:   # (a raw block, when libzstd wrote one)
            bad = flip(f, raw[0][1] + 7, 2)
            assert vbz.decompress_raw(bad, a.nbytes, opts) == E_ZSTD


# ---- 3. the writer ----------------------------------------------------------------------------------------------------------------------
def _content(a, size, zigzag, version):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1) if size == 0 else O.svb_compress(a, size, zigzag, version)


def _check_written(outs, reads, opts, size, zigzag, version):
    L = _lib.load()
    for g, a in zip(outs, reads):
        assert not isinstance(g, int), g
        assert len(g) <= L.vbz_max_compressed_size(a.nbytes, ctypes.byref(opts))
        assert g[4] & 4, "Content_Checksum_flag"
        end, _ = blocks_end(g)
        content = _content(a, size, zigzag, version)
        assert int(g[end : end + 4].view("<u4")[0]) == xxh64(content) & 0xFFFFFFFF
        dec = O.zstd_decompress(g, content.nbytes + 64)   # libzstd verifies the checksum
        assert dec is not None and dec.tobytes() == content.tobytes()
    back = G.decompress(outs, [a.nbytes for a in reads], opts)
    for b, a in zip(back, reads):
        assert not isinstance(b, int) and b.tobytes() == a.tobytes()


def _typed(a, size):
    return {0: a.view(np.uint8), 1: (a & 0x7F).astype(np.int8), 2: a, 4: a.astype(np.int32) * 3}[size]


@pytest.mark.parametrize("size", [0, 1, 2, 4])
@pytest.mark.parametrize("zigzag", [False, True])
@pytest.mark.parametrize("version", [0, 1])
def test_writer_every_option(size, zigzag, version, checksum_on):
    if size == 0 and (zigzag or version):
        pytest.skip("integer_size 0 has no svb options")
    rng = np.random.default_rng(size * 4 + zigzag * 2 + version)
    lens = [0, 1, 5, 77, 1000, 4099] + rng.integers(100, 60000, 40).tolist()
    reads = [_typed(O.synth_signal(9, i, n), size) for i, n in enumerate(lens)]
    opts = _lib.CompressionOptions(zigzag, size, 1, version)
    _check_written(G.compress(reads, opts), reads, opts, size, zigzag, version)


def test_writer_bench_shape_large_reads_trailers_canonical(checksum_on):
    c = checksum_on
    opts = _lib.CompressionOptions(True, 2, 1, 1)
    reads = [O.synth_signal(5, i, 90000 + (i * 7919) % 20001) for i in range(600)]
    outs = G.compress(reads, opts)
    _check_written(outs, reads, opts, 2, True, 1)
    n, b, w = c.decode_paths()
    assert n == len(reads) and b == n, "own frames with checksums on the batched decoder"
    big = [O.synth_signal(5, 9999, 4_000_000)]
    outs = G.compress(big, opts)
    _check_written(outs, big, opts, 2, True, 1)
    assert c.decode_span_paths() == (1, 1), "decoded span by span"
    # a long read routed beside ordinary ones
    mixed = reads[:64] + [O.synth_signal(5, 8888, 700_000)]
    _check_written(G.compress(mixed, opts), mixed, opts, 2, True, 1)
    # raw blocks of incompressible bytes around the 128 KiB block boundaries
    rng = np.random.default_rng(4)
    raw = [rng.integers(0, 256, n, dtype=np.uint8) for n in (131071, 131072, 131073, 262144, 262145, 1 << 20)]
    o0 = _lib.CompressionOptions(False, 0, 1, 0)
    _check_written(G.compress(raw, o0), raw, o0, 0, False, 0)
    c.set_trailers(0)
    _check_written(G.compress(reads[:50] + big, opts), reads[:50] + big, opts, 2, True, 1)
    c.set_trailers(1)
    c.set_canonical(1)
    _check_written(G.compress(mixed, opts), mixed, opts, 2, True, 1)


def test_writer_adds_only_the_checksum(fresh_codec):
    """on and off in one context: the frame with the checksum is the frame without it plus the flag and the four bytes behind the last
    block (trailers and all), and off writes no flag"""
    c = fresh_codec
    opts = _lib.CompressionOptions(True, 2, 1, 1)
    reads = [O.synth_signal(5, i, 30000 + 997 * i) for i in range(20)] + [O.synth_signal(5, 99, 700_000)]
    off = G.compress(reads, opts)
    c.set_checksum(1)
    on = G.compress(reads, opts)
    c.set_checksum(0)
    again = G.compress(reads, opts)
    for f, g, h in zip(off, on, again):
        assert not f[4] & 4 and f.tobytes() == h.tobytes()
        end, _ = blocks_end(g)
        stripped = np.concatenate([g[:end], g[end + 4 :]])
        stripped[4] &= ~4 & 0xFF
        assert stripped.tobytes() == f.tobytes()


# ---- 4. own frames with a damaged checksum ------------------------------------------------------------------------------------------------
def test_own_frame_damaged_checksum(checksum_on):
    opts = _lib.CompressionOptions(True, 2, 1, 1)
    reads = [O.synth_signal(5, i, 50000 + i) for i in range(30)] + [O.synth_signal(5, 77, 2_000_000)]
    outs = G.compress(reads, opts)
    bad = set()
    damaged = []
    for i, g in enumerate(outs):
        if i % 3 == 0:
            end, _ = blocks_end(g)
            g = flip(g, end + i % 4, i % 8)
            bad.add(i)
            assert O.zstd_decompress(g, reads[i].nbytes * 3) is None
        damaged.append(g)
    got = G.decompress(damaged[:-1], [a.nbytes for a in reads[:-1]], opts)
    _check_verdicts(got, damaged[:-1], reads[:-1], bad)
    got = G.decompress(damaged[-1:], [reads[-1].nbytes], opts)
    assert got[0] == E_ZSTD


# ---- 5. the environment variable, in a fresh process ----------------------------------------------------------------------------------------
def test_env_knob_single_buffer(tmp_path):
    out = tmp_path / "c.bin"
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import numpy as np, oracle_lib as O\nfrom vbz_compression_amd import vbz\n"
            "a = O.synth_signal(5, 3, 70000)\nopen(%r, 'wb').write(vbz.compress(a).tobytes())\n" % (ROOT, os.path.join(ROOT, "tests"), str(out)))
    env = dict(os.environ, VBZ_HIP_CHECKSUM="1")
    subprocess.run([sys.executable, "-c", code], env=env, check=True, timeout=600)
    c = np.frombuffer(out.read_bytes(), np.uint8)
    a = O.synth_signal(5, 3, 70000)
    frame = c[4:]   # the sized header
    assert frame[4] & 4
    dec = O.zstd_decompress(frame, a.nbytes * 3)
    assert dec is not None and dec.tobytes() == O.svb_compress(a, 2, True, 0).tobytes()


def test_stage_writer_never_returns_a_frame_without_checksum(checksum_on):
    """vbz_gpu_zstd_compress_batch with slots too small for the checksum: VBZ_DESTINATION_SIZE_ERROR (or the encoder's own verdict),
    never a frame without it"""
    c = checksum_on
    c.set_trailers(0)
    base = [O.svb_compress(O.synth_signal(5, i, 20000 + 313 * i), 2, True, 0) for i in range(6)]
    c.set_checksum(0)
    plain = G.zstd_compress(base)
    room = [0, 1, 2, 3, 4, 8, 16, 32, 64, 128, 256, 512]
    streams = [s for s in base for k in room]
    caps = [len(f) + k for f in plain for k in room]
    off = G.run_stage(lambda cc, *a: cc.zstd_compress(*a), streams, caps)
    c.set_checksum(1)
    on = G.run_stage(lambda cc, *a: cc.zstd_compress(*a), streams, caps)
    tight = 0
    for f, g, cap, s in zip(off, on, caps, streams):
        if isinstance(g, int):
            assert g == _lib.VBZ_DESTINATION_SIZE_ERROR or isinstance(f, int), (g, f)
            if not isinstance(f, int):   # the frame fitted, the checksum did not
                assert len(f) + 4 > cap
                tight += 1
            continue
        assert g[4] & 4 and len(g) <= cap
        assert O.zstd_decompress(g, s.nbytes + 16).tobytes() == s.tobytes()
    assert any(not isinstance(g, int) for g in on)
