"""The normalising decode on the MI355X (include/vbz_gpu.h: vbz_gpu_signal_norm_batch, vbz_gpu_decompress_signal_norm_batch,
vbz_gpu_decompress_chunks_norm_batch; batch.GpuCodec.signal_norm and norm= of the signal and chunk decodes).  Every read's (shift, scale)
is held bit for bit to the numpy statement of tests/norm_ref.py, the normalised samples to numpy's conversion with those constants, the
normalised chunks byte for byte to the chunk call fed the same constants, and every verdict to the int16 decode's -- on every decode path."""
import ctypes

import numpy as np
import pytest
import torch

import norm_ref as R
import oracle_lib as O
from signal_ref import typed_bits
from typed_support import ELEM, Frames, arena, check_stats, codec, int16, key, norm_of, stats, u32, walk_signal
from vbz_compression_amd import _lib, batch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]


# ---- reads ------------------------------------------------------------------------------------------------------------------
def mixed_reads(seed, signed=True, long_len=100_003):
    """every kind of read the statistics must be exact for"""
    rng = np.random.default_rng(seed)
    out = []
    for T in (0, 1, 2, 3, 8, 999, 1000, 4096, 20_001, long_len):
        out.append(walk_signal(rng, T))
        out.append(rng.integers(-32768, 32768, T).astype(np.int16))           # full-range noise: every stage falls back
        out.append(np.full(T, rng.integers(-32768, 32768), np.int16))         # constant
        two = np.where(rng.random(T) < 0.5, -30000, 31000).astype(np.int16)   # two values far apart
        out.append(two)
        far = walk_signal(rng, T)                                             # a far outlier first: the first window misses
        if T:
            far[0] = -31000
        out.append(far)
        out.append(np.where(rng.random(T) < 0.3, 400, 200).astype(np.int16))   # two values, close
    if not signed:
        out = [(x.astype(np.int32) & 0xFFFF).astype(np.uint16) for x in out]
        rng2 = np.random.default_rng(seed + 99)
        out.append(rng2.integers(0, 65536, 5000).astype(np.uint16))
        out.append(np.full(77, 65535, np.uint16))
    return out


def compress_oracle(c, reads, oopts, sized=False):
    return arena(c, [O.compress(x.view(np.int16), oopts, sized=sized) for x in reads], 64)


# ---- 1. the statistics --------------------------------------------------------------------------------------------------------
OPTS = [(True, 1, 1, False), (True, 1, 0, False), (True, 0, 1, True), (False, 1, 1, False), (True, 1, 1, True), (False, 0, 0, True)]


@pytest.mark.parametrize("zz,level,version,sized", OPTS)
@pytest.mark.parametrize("pi", range(len(R.PARAMS)))
def test_stats_exact(zz, level, version, sized, pi):
    case = Frames(codec(), mixed_reads(7 + pi), _lib.CompressionOptions(zz, 2, level, version), sized)
    check_stats(case, R.PARAMS[pi])


@pytest.mark.parametrize("pi", range(len(R.PARAMS)))
def test_stats_uint16(pi):
    case = Frames(codec(), mixed_reads(11, signed=False), _lib.CompressionOptions(True, 2, 1, 1))
    check_stats(case, R.PARAMS[pi], signed=False)


# ---- 2. signal decode ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pi", [0, 1])
@pytest.mark.parametrize("signed", [True, False])
def test_signal_norm(dtype, pi, signed):
    c = codec()
    reads = mixed_reads(21, signed=signed, long_len=30_001)
    case = Frames(codec(), reads, _lib.CompressionOptions(True, 2, 1, 1))
    p = R.PARAMS[pi]
    E = ELEM[key(dtype)]
    n = case.n
    out = torch.zeros((case.dst_bytes // 2 + 64), dtype=dtype, device=c.device)
    res = torch.zeros(n, dtype=torch.int32, device=c.device)
    ss = torch.zeros((n, 2), dtype=torch.float32, device=c.device)
    c.decompress_signal(case.src, case.off, case.size, out, case.doff // 2 * E, (case.dcap // 2) * E, res, case.opts, signed=signed,
                        norm=norm_of(p), norm_out=ss)
    torch.cuda.synchronize()
    res = u32(res)
    ss = ss.cpu().numpy()
    bits = out.view(torch.int32 if E == 4 else torch.int16).cpu().numpy().view(np.uint32 if E == 4 else np.uint16)
    offs = (case.doff // 2).cpu().numpy()
    for i, x in enumerate(reads):
        assert res[i] == len(x) * E, (i, res[i])
        shift, scale, o, s = R.constants(*R.stats(x, p), p)
        assert ss[i][0] == shift and ss[i][1] == scale
        got = bits[offs[i] : offs[i] + len(x)]
        want = typed_bits(x.view(np.int16) if signed else x, o, s, key(dtype))
        assert (got == want).all(), (i, len(x))


# ---- 3. chunks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,end_align", [("pad", 0), ("end", 8), ("end", 1)])
@pytest.mark.parametrize("pi", [0, 1])
def test_chunks_norm(mode, end_align, pi):
    c = codec()
    reads = mixed_reads(31, long_len=40_000)
    case = Frames(codec(), reads, _lib.CompressionOptions(True, 2, 1, 1))
    samples = torch.tensor(case.T, dtype=torch.int32, device=c.device)
    ss = torch.zeros((case.n, 2), dtype=torch.float32, device=c.device)
    res_n = torch.zeros(case.n, dtype=torch.int32, device=c.device)
    ch_n, first_n, _ = c.decompress_chunks(case.src, case.off, case.size, samples, res_n, case.opts, 1000, 504, mode, max(end_align, 1),
                                           pad=0.0, dtype=torch.float16, norm=norm_of(R.PARAMS[pi]), norm_out=ss)
    torch.cuda.synchronize()
    offset = (-ss[:, 0]).contiguous()
    scale = (1.0 / ss[:, 1].double()).float().contiguous()
    res_p = torch.zeros(case.n, dtype=torch.int32, device=c.device)
    ch_p, first_p, _ = c.decompress_chunks(case.src, case.off, case.size, samples, res_p, case.opts, 1000, 504, mode, max(end_align, 1),
                                           pad=0.0, dtype=torch.float16, scale=scale, offset=offset)
    torch.cuda.synchronize()
    assert (u32(res_n) == u32(res_p)).all()
    assert torch.equal(first_n, first_p)
    assert torch.equal(ch_n.view(torch.int16), ch_p.view(torch.int16))
    sh = ss.cpu().numpy()
    for i, x in enumerate(reads):
        want = R.shift_scale(x, R.PARAMS[pi])
        assert sh[i][0] == want[0] and sh[i][1] == want[1], i


# ---- 4. every path ------------------------------------------------------------------------------------------------------------
def small_reads(seed, n, lo=50, hi=400):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        T = int(rng.integers(lo, hi))
        out.append(walk_signal(rng, T) if i % 3 else rng.integers(-32768, 32768, T).astype(np.int16))
    return out


@pytest.mark.parametrize("pi", [0, 1])
def test_split_batch(pi):
    case = Frames(codec(), small_reads(41, 16_500), _lib.CompressionOptions(True, 2, 1, 1))
    check_stats(case, R.PARAMS[pi])


@pytest.mark.parametrize("pi", [0, 1])
def test_routed_long_reads(pi):
    rng = np.random.default_rng(51)
    reads = small_reads(52, 600, 1000, 3000)
    far = walk_signal(rng, 300_000)
    far[0] = 30000
    reads[100] = far
    reads[400] = rng.integers(-32768, 32768, 280_000).astype(np.int16)
    reads[500] = walk_signal(rng, 400_001)
    case = Frames(codec(), reads, _lib.CompressionOptions(True, 2, 1, 1))
    check_stats(case, R.PARAMS[pi])


@pytest.mark.parametrize("pi", [0, 1, 2])
def test_large_read_path(pi):
    rng = np.random.default_rng(61)
    reads = [walk_signal(rng, 400_000), rng.integers(-32768, 32768, 400_001).astype(np.int16), np.full(400_000, -5, np.int16)]
    far = walk_signal(rng, 399_999)
    far[0] = -32000
    reads.append(far)
    check_stats(Frames(codec(), reads, _lib.CompressionOptions(True, 2, 1, 1)), R.PARAMS[pi])
    check_stats(Frames(codec(), reads, _lib.CompressionOptions(True, 2, 0, 1), sized=True), R.PARAMS[pi])


def test_one_huge_read():
    rng = np.random.default_rng(71)
    x = walk_signal(rng, 20_000_000)
    case = Frames(codec(), [x], _lib.CompressionOptions(True, 2, 1, 1))
    for p in (R.BONITO, R.DORADO):
        check_stats(case, p)
    # counts above 2^16 per value, and the fallback: values far from the first sample
    y = np.where(rng.random(20_000_000) < 0.5, -20000, 25000).astype(np.int16)
    y[0] = 0
    check_stats(Frames(codec(), [y], _lib.CompressionOptions(True, 2, 1, 1)), R.BONITO)


@pytest.mark.parametrize("pi", [0, 1])
def test_libzstd_frames(pi):
    reads = mixed_reads(81, long_len=50_000)
    oo = O.options(True, 2, 1, 1)
    case = Frames(codec(), reads, _lib.CompressionOptions(True, 2, 1, 1), sized=True, comp=compress_oracle(codec(), reads, oo, sized=True))
    check_stats(case, R.PARAMS[pi])


def test_checksummed_frames():
    c = codec()
    c.set_checksum(1)
    try:
        case = Frames(codec(), mixed_reads(91, long_len=60_000), _lib.CompressionOptions(True, 2, 1, 1))
    finally:
        c.set_checksum(0)
    check_stats(case, R.BONITO)
    check_stats(case, R.DORADO)


# ---- 5. errors among good reads -----------------------------------------------------------------------------------------------
def test_damaged_frames_and_bad_descriptors():
    c = codec()
    reads = mixed_reads(101, long_len=20_000)
    case = Frames(codec(), reads, _lib.CompressionOptions(True, 2, 1, 1))
    src = case.src.clone()
    offs = case.off.cpu().numpy()
    sizes = u32(case.size)
    bad = set()
    for i in range(5, case.n, 7):   # damage the middle of some frames
        if sizes[i] > 16:
            o = int(offs[i]) + int(sizes[i]) // 2
            src[o : o + 4] ^= 0x5A
            bad.add(i)
    case.src = src
    cap = case.dcap.clone()
    for i in range(3, case.n, 11):   # wrong capacity: a destination size error
        if case.T[i] > 0:
            cap[i] = cap[i] + 2
            bad.add(i)
    case.dcap = cap
    for p in (R.BONITO, R.DORADO):
        ss, res = stats(case, p)
        want = int16(case)
        assert (res == want).all()
        for i, x in enumerate(reads):
            if _lib.is_error(int(res[i])) or i in bad:
                continue
            shift, scale = R.shift_scale(x, p)
            assert ss[i][0] == shift and ss[i][1] == scale, i


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals():
    c = codec()
    L = c.L
    reads = mixed_reads(111, long_len=1000)[6:12]   # (one sample each)
    case = Frames(codec(), reads, _lib.CompressionOptions(True, 2, 1, 1))
    n = case.n
    ss = torch.full((n, 2), 7.0, dtype=torch.float32, device=c.device)
    res = torch.full((n,), 12345, dtype=torch.int32, device=c.device)
    out = torch.full((case.dst_bytes // 2 + 64,), 3.0, dtype=torch.float16, device=c.device)
    b = c._batch(case.src, case.off, case.size, out.view(torch.uint8), case.doff, case.dcap, res)
    opts = case.opts
    f = _lib.GpuSignalFormat()
    f.out_type, f.is_signed = _lib.VBZ_GPU_SIGNAL_F16, 1
    ch = c._chunking(1000, 504, "pad", 0)
    chunk_first = torch.zeros(n + 1, dtype=torch.int64, device=c.device)
    chunks = torch.zeros((8, 1000), dtype=torch.float16, device=c.device)

    def good():
        return batch.MED_MAD.c_struct()

    def calls(m, fmt=f, o=opts, ssp=ss.data_ptr()):
        mp = ctypes.byref(m) if m is not None else None
        return [
            L.vbz_gpu_signal_norm_batch(c.ctx, ctypes.byref(b), ctypes.byref(o), 0, 1, mp, ssp),
            L.vbz_gpu_decompress_signal_norm_batch(c.ctx, ctypes.byref(b), ctypes.byref(o), 0, ctypes.byref(fmt), mp, ssp),
            L.vbz_gpu_decompress_chunks_norm_batch(c.ctx, ctypes.byref(b), ctypes.byref(o), 0, ctypes.byref(fmt), ctypes.byref(ch),
                                                   chunk_first.data_ptr(), chunks.data_ptr(), 8, mp, ssp),
        ]

    def mutate(**kw):
        m = good()
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    inf, nan = float("inf"), float("nan")
    bad = [None, mutate(method=0), mutate(method=3), mutate(reserved=1), mutate(quantile_a=0.1), mutate(quantile_b=0.5),
           mutate(method=2, quantile_a=0.6, quantile_b=0.5), mutate(method=2, quantile_a=-0.1, quantile_b=0.5),
           mutate(method=2, quantile_a=0.1, quantile_b=1.5), mutate(method=2, quantile_a=nan, quantile_b=0.5),
           mutate(shift_mul=nan), mutate(shift_mul=inf), mutate(scale_mul=-inf), mutate(shift_min=inf), mutate(shift_min=nan),
           mutate(scale_min=0.0), mutate(scale_min=-1.0), mutate(scale_min=1e-40), mutate(scale_min=inf), mutate(scale_min=nan)]
    for m in bad:
        rcs = calls(m)
        assert rcs == [-2, -2, -2], (m and [getattr(m, k[0]) for k in m._fields_], rcs)
        assert L.vbz_gpu_last_error(c.ctx).decode() != ""
    # a format with constants, unknown options, a NULL shift_scale for the statistics alone
    scale = torch.ones(n, dtype=torch.float32, device=c.device)
    f2 = _lib.GpuSignalFormat()
    f2.out_type, f2.is_signed, f2.scale = _lib.VBZ_GPU_SIGNAL_F16, 1, scale.data_ptr()
    assert calls(good(), fmt=f2, ssp=None)[1:] == [-2, -2]   # (the statistics alone take no format: only their NULL shift_scale is refused)
    assert calls(good(), o=_lib.CompressionOptions(True, 4, 1, 1)) == [-2, -2, -2]
    assert L.vbz_gpu_signal_norm_batch(c.ctx, ctypes.byref(b), ctypes.byref(opts), 0, 2, ctypes.byref(good()), ss.data_ptr()) == -2
    assert L.vbz_gpu_signal_norm_batch(c.ctx, ctypes.byref(b), ctypes.byref(opts), 0, 1, ctypes.byref(good()), None) == -2
    assert L.vbz_gpu_last_error(c.ctx).decode() != ""
    assert L.vbz_gpu_signal_norm_batch(None, ctypes.byref(b), ctypes.byref(opts), 0, 1, ctypes.byref(good()), ss.data_ptr()) == -1
    torch.cuda.synchronize()
    assert (ss.cpu() == 7.0).all() and (res.cpu() == 12345).all() and (out.cpu() == 3.0).all() and (chunks.cpu() == 0).all()
