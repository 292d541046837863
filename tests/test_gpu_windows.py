"""Caller-listed signal windows on the MI355X (include/vbz_gpu.h: vbz_gpu_windows and the two *_windows_batch calls).  Every case is held
bit for bit to tests/windows_ref.py, with the arena filled with a canary and checked outside the passing reads' rows, guard rows behind it:
sizes around a lane (8 samples), a wavefront (512), a tile (2 048) and the paired-tile loop crossed with starts in front of, at, inside,
at the end of and behind the signal; dense overlap and long lists; the tie to the chunk call; every output type and option; ranges and
normalisation; the large-read path, split and routed call shapes, libzstd's and checksummed frames; POD5 rows and reads; verdicts."""
import numpy as np
import pytest
import torch

import norm_ref as R
import oracle_lib as O
import pod5_reads_ref as PR
import ranges_ref as G
import signal_ref as SR
from typed_support import CANARY, ELEM, NORMS, Frames, arena, codec, expect_results, frames_of, i32, sine_signal, u32
from vbz_compression_amd import _lib, batch
from windows_support import WinCall, WinRun

pytestmark = pytest.mark.gpu

E_ZSTD, E_INPUT, E_DEST, E_STREAM = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFC, 0xFFFFFFFB
TO_END = 0xFFFFFFFF


def consts(rng, n):
    return rng.uniform(-600, 600, n).astype(np.float32), rng.uniform(0.01, 2.5, n).astype(np.float32)


def random_starts(rng, T, L, k):
    """k sorted starts from just in front of the signal to just behind it, every third a multiple of 8"""
    v = rng.integers(-L, T + L + 1, k)
    v[::3] &= ~7
    return sorted(int(x) for x in v)


# ---- 1. sizes x starts ----------------------------------------------------------------------------------------------------------------------
SIZES = [0, 1, 7, 8, 9, 511, 513, 2047, 2048, 2049, 4095, 4097, 20_000]


def starts_of(T, L):
    return sorted([-L + 1, -8, -3, 0, 0, 1, 7, 8, 9, 504, 509, 2040, 2047, 2048, T - L, T - L + 3, T - 1, T, T + 5])


_grid = {}


def grid(c):
    if "g" not in _grid:
        rng = np.random.default_rng(17)
        reads = [sine_signal(rng, T) if k % 3 else rng.integers(-32768, 32768, T).astype(np.int16) for k, T in enumerate(SIZES)]
        _grid["g"] = Frames(c, reads, c.options(True, 2, 1, 1))
    return _grid["g"]


@pytest.mark.parametrize("L", [8, 16, 1024, 4096])
def test_sizes_and_starts(L):
    c = codec()
    fr = grid(c)
    o, s = consts(np.random.default_rng(L), fr.n)
    starts = [starts_of(T, L) for T in fr.T]
    for dtype in ("f32", "f16", "bf16"):
        for signed in (True, False):
            WinRun(fr, starts, L, dtype, signed=signed, offset=o, scale=s).check()


# ---- 2. dense overlap and long lists ----------------------------------------------------------------------------------------------------------
def test_dense_overlap_and_long_lists():
    c = codec()
    rng = np.random.default_rng(19)
    reads = [sine_signal(rng, T) for T in (3000, 900, 500, 0, 1200, 5000)]
    starts = [list(range(700)), random_starts(rng, 900, 16, 5), [], [0, 3], random_starts(rng, 1200, 16, 9), [8 * k - 40 for k in range(700)]]
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    o, s = consts(rng, fr.n)
    for dtype in ("f16", "f32"):
        WinRun(fr, starts, 16, dtype, offset=o, scale=s).check()
    WinRun(fr, [list(range(0, 2800, 4)), [], [], [-5, -5], [100] * 70, list(range(-100, 5100, 64))], 512, "bf16", offset=o, scale=s).check()


# ---- 3. the tie to the chunk call -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,S", [(16, 8), (1024, 1000)])
def test_pad_grid_is_the_chunk_call(L, S):
    c = codec()
    fr = grid(c)
    dev = c.device
    samples = i32(fr.T).to(dev)
    o, s = consts(np.random.default_rng(S), fr.n)
    od, sd = torch.from_numpy(o).to(dev), torch.from_numpy(s).to(dev)
    res = torch.full((fr.n,), -8, dtype=torch.int32, device=dev)
    chunks, chunk_first, info = c.decompress_chunks(fr.src, fr.off, fr.size, samples, res, fr.opts, L, S, "pad", 0, -7.0, torch.float16, scale=sd, offset=od)
    torch.cuda.synchronize()
    assert u32(res).tolist() == [2 * T for T in fr.T]
    res2 = torch.full((fr.n,), -8, dtype=torch.int32, device=dev)
    start = info[:, 1].contiguous()
    out = c.decompress_windows(fr.src, fr.off, fr.size, samples, res2, fr.opts, chunk_first, start, L, -7.0, torch.float16, scale=sd, offset=od)
    torch.cuda.synchronize()
    assert u32(res2).tolist() == [2 * T for T in fr.T]
    assert tuple(out.shape) == tuple(chunks.shape) and out.dtype == chunks.dtype
    assert out.cpu().numpy().tobytes() == chunks.cpu().numpy().tobytes()
    assert start.cpu().tolist() == [v for T in fr.T for v in SR.chunk_starts(T, L, S, "pad", 0)]
    # the same through the method with norm=: the tensor and shift_scale
    out2, ss = c.decompress_windows(fr.src, fr.off, fr.size, samples, res2, fr.opts, chunk_first, start, L, -7.0, torch.float16, norm=batch.MED_MAD)
    ch2, _, _ = c.decompress_chunks(fr.src, fr.off, fr.size, samples, res, fr.opts, L, S, "pad", 0, -7.0, torch.float16, norm=batch.MED_MAD)
    torch.cuda.synchronize()
    assert out2.cpu().numpy().tobytes() == ch2.cpu().numpy().tobytes() and tuple(ss.shape) == (fr.n, 2)


# ---- 4. options ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sized", [False, True], ids=["unsized", "sized"])
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("version", [0, 1])
@pytest.mark.parametrize("zz", [True, False], ids=["zz", "nozz"])
def test_output_types_and_options(zz, version, level, sized):
    c = codec()
    rng = np.random.default_rng(version * 8 + level * 4 + sized * 2 + zz)
    reads = [sine_signal(rng, T) if (zz and k % 2) else rng.integers(-32768, 32768, T).astype(np.int16) for k, T in enumerate([0, 1, 7, 9, 513, 2049, 4101, 20_000])]
    fr = Frames(c, reads, c.options(zz, 2, level, version), sized, slack=6)
    o, s = consts(rng, fr.n)
    starts = [random_starts(rng, T, 1024, 12) for T in fr.T]
    for dtype in ("f32", "f16", "bf16"):
        for signed in (True, False):
            WinRun(fr, starts, 1024, dtype, signed=signed, offset=o, scale=s).check()
    WinRun(fr, [starts_of(T, 16) for T in fr.T], 16, "f32", [8, 3] * 4, [TO_END] * 8, norm=NORMS["med_mad"], signed=False).check()


# ---- 5. ranges and normalisation ------------------------------------------------------------------------------------------------------------------
def range_case():
    rng = np.random.default_rng(29)
    reads, bg, en = [], [], []
    for T in (0, 1, 9, 513, 2049, 4101, 20_000):
        x = sine_signal(rng, T)
        for b, e in ((8, T - 3 if T > 3 else T), (3, TO_END), (8, TO_END), (3, max(T - 100, 0)), (2048, 2048), (TO_END, 0), (0, T)):
            reads.append(x)
            bg.append(b)
            en.append(e)
    return reads, bg, en


@pytest.mark.parametrize("L", [16, 1024])
def test_ranges(L):
    c = codec()
    reads, bg, en = range_case()
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    rng = np.random.default_rng(L)
    o, s = consts(rng, fr.n)
    Tp = [G.clamp(T, b, e) for T, b, e in zip(fr.T, bg, en)]
    starts = [sorted(starts_of(e - b, L)[:10] + random_starts(rng, e - b, L, 6)) for b, e in Tp]
    for dtype in ("f16", "f32", "bf16"):
        WinRun(fr, starts, L, dtype, bg, en, offset=o, scale=s).check()
    WinRun(fr, starts, L, "f16", bg, None, offset=o, scale=s).check()
    WinRun(fr, starts, L, "f16", None, en, offset=o, scale=s).check()


@pytest.mark.parametrize("stats", [0, 1], ids=["range", "read"])
@pytest.mark.parametrize("method", ["med_mad", "quantile"])
def test_normalised_windows(method, stats):
    c = codec()
    reads, bg, en = range_case()
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    rng = np.random.default_rng(3)
    starts = [random_starts(rng, T, 1024, 8) for T in fr.T]
    WinRun(fr, starts, 1024, "f16", bg, en, norm=NORMS[method], stats=stats).check()
    WinRun(fr, starts, 1024, "f32", norm=NORMS[method], stats=stats).check()   # (no ranges: the whole read either way)


# ---- 6. the other decode paths ------------------------------------------------------------------------------------------------------------------------
SEG = 16_384


def large_read_checks(c):
    rng = np.random.default_rng(23)
    x = sine_signal(rng, 40_000)
    x[:3000] += 3000
    fr = Frames(c, [x], c.options(True, 2, 1, 1))
    for L in (16, 1024, 4096):
        st = sorted([-L + 5, -8, 0, 3, SEG - L, SEG - L + 1, SEG - 8, SEG - 3, SEG, SEG + 1, 2 * SEG - L // 2, 2 * SEG - 8, 2 * SEG - 1, 2 * SEG, 2 * SEG + 8,
                     40_000 - L, 40_000 - L + 8, 40_000 - 5, 40_000, 41_000] + random_starts(rng, 40_000, L, 40))
        WinRun(fr, [st], L, ["f16", "f32", "bf16"][L % 3], offset=[-37.5], scale=[0.173]).check()
        WinRun(fr, [st], L, "f16", [SEG - 5], [2 * SEG + 100], norm=NORMS["med_mad" if L == 16 else "quantile"], stats=L // 1024 % 2).check()
    WinRun(fr, [list(range(SEG - 400, SEG + 400))], 64, "f16").check()


def test_one_large_read_alone_in_a_call():
    large_read_checks(codec())


@pytest.mark.parametrize("segmented", [1, 0])
def test_large_read_on_forced_paths(segmented):
    large_read_checks(codec(VBZ_HIP_SEGMENTED=segmented))


def small_batch(seed, n, L, lo=50, hi=3000):
    rng = np.random.default_rng(seed)
    reads, starts = [], []
    for i in range(n):
        T = int(rng.integers(lo, hi))
        reads.append(sine_signal(rng, T) if i % 3 else rng.integers(-32768, 32768, T).astype(np.int16))
        starts.append(random_starts(rng, T, L, int(rng.integers(0, 7))))
    return reads, starts


def test_split_batch():
    reads, starts = small_batch(31, 200, 1024)
    outs = []
    for c in (codec(VBZ_HIP_SPLIT_MIN=64), codec(VBZ_HIP_SPLIT_MIN=0)):
        fr = Frames(c, reads, c.options(True, 2, 1, 1))
        r = WinRun(fr, starts, 1024, "f16", norm=NORMS["med_mad"]).check()
        outs.append((r.out.cpu().numpy().tobytes(), r.ss.cpu().numpy().tobytes()))
        WinRun(fr, starts, 16, "bf16").check()
    assert outs[0] == outs[1]


def test_routed_long_read_among_small_ones():
    c = codec()
    reads, starts = small_batch(41, 600, 4096, 500, 5000)
    rng = np.random.default_rng(42)
    reads[100] = sine_signal(rng, 300_000)
    starts[100] = sorted([-100, 0, 8, 299_000, 299_999, 300_000] + random_starts(rng, 300_000, 4096, 60))
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    o, s = consts(rng, fr.n)
    WinRun(fr, starts, 4096, "f16", offset=o, scale=s).check()
    bg, en = [8 if i % 2 else 3 for i in range(fr.n)], [TO_END if i % 3 else 2000 for i in range(fr.n)]
    bg[100], en[100] = 2003, 298_000
    WinRun(fr, starts, 4096, "f32", bg, en, norm=NORMS["quantile"], stats=1).check()


def other_frames_reads():
    rng = np.random.default_rng(51)
    reads = [sine_signal(rng, T) for T in (0, 1, 9, 2049, 4101, 50_000)]
    return reads, [random_starts(rng, len(x), 1024, 14) for x in reads]


def test_libzstd_frames():
    c = codec()
    reads, starts = other_frames_reads()
    comp = arena(c, [O.compress(x, O.options(True, 2, 1, 1), sized=True) for x in reads], 64)
    fr = Frames(c, reads, c.options(True, 2, 1, 1), sized=True, comp=comp)
    WinRun(fr, starts, 1024, "f16", norm=NORMS["med_mad"]).check()
    WinRun(fr, starts, 1024, "f32", [8] * fr.n, [TO_END] * fr.n).check()


def test_checksummed_frames():
    c = codec()
    reads, starts = other_frames_reads()
    c.set_checksum(1)
    try:
        fr = Frames(c, reads, c.options(True, 2, 1, 1))
    finally:
        c.set_checksum(0)
    WinRun(fr, starts, 1024, "bf16", norm=NORMS["quantile"]).check()
    WinRun(fr, starts, 1024, "f16").check()


# ---- 7. POD5 ------------------------------------------------------------------------------------------------------------------------------------
POD5_SHAPES = [[13, 7, 1, 2047, 2049], [800, 0, 800], [24, 8, 2056, 16], [300] * 40, []]


def test_pod5_rows_as_reads_of_their_own():
    c = codec()
    lens = [0, 1, 7, 9, 513, 2047, 2049, 4101, 20_000]
    rows, first, frames = frames_of(73, [[n] for n in lens for _ in range(2)])
    fr = Frames(c, rows, batch.pod5_options(), comp=arena(c, frames, 64))
    rng = np.random.default_rng(7)
    o, s = consts(rng, fr.n)
    for L, dtype in ((16, "f16"), (1024, "f32"), (1024, "bf16")):
        WinRun(fr, [starts_of(T, L) for T in fr.T], L, dtype, offset=o, scale=s).check()
    WinRun(fr, [random_starts(rng, T, 1024, 9) for T in fr.T], 1024, "f16", [8, 3] * len(lens), [TO_END, 4000] * len(lens), norm=NORMS["med_mad"]).check()


def pod5_windows(rng, lens, L, b=0, e=None):
    """windows across the row boundaries and the ends of a read's range"""
    T = sum(lens)
    e = T if e is None else min(e, T)
    b = min(b, e)
    cum = np.cumsum([0] + lens).tolist()
    st = [-L + 1, -3, 0, e - b - L, e - b - 1, e - b, e - b + 5] + [v - b - k for v in cum for k in (0, 3, 8, L // 2)]
    return sorted(st + random_starts(rng, e - b, L, 5))


@pytest.mark.parametrize("segmented", [0, 1])
@pytest.mark.parametrize("L", [8, 16, 1024])
def test_pod5_reads(segmented, L):
    c = codec(VBZ_HIP_SEGMENTED=segmented)
    shapes = POD5_SHAPES * 2
    rows, first, frames = frames_of(71, shapes)
    rng = np.random.default_rng(L)
    n = len(first)
    o, s = consts(rng, n)
    starts = [pod5_windows(rng, lens, L) for lens in shapes]
    for dtype in (("f32", "f16", "bf16") if L == 16 else ("f16",)):
        call = WinCall(c, frames, rows, first, starts, L, dtype, offset=o, scale=s)
        assert call.call() == 0, c.L.vbz_gpu_last_error(c.ctx)
        expect_results(call, rows, first, ELEM[dtype])
        call.check(consts=list(zip(o, s)))
    # ranges: begins at 8 and 3, ends inside and to the end, an empty one
    bg = [8, 3, 8, 3, 0, 8, 3, 2000, 700, TO_END]
    en = [TO_END, 3000, 1000, TO_END, 0, 4000, TO_END, 2100, 20, 0]
    starts = [pod5_windows(rng, lens, L, b, e) for lens, b, e in zip(shapes, bg, en)]
    call = WinCall(c, frames, rows, first, starts, L, "f16", bg, en, offset=o, scale=s)
    assert call.call() == 0, c.L.vbz_gpu_last_error(c.ctx)
    expect_results(call, rows, first, 2)
    call.check(consts=list(zip(o, s)))
    for stats in (0, 1):
        call = WinCall(c, frames, rows, first, starts, L, "f16", bg, en, norm=batch.MED_MAD, stats=stats)
        assert call.call() == 0, c.L.vbz_gpu_last_error(c.ctx)
        expect_results(call, rows, first, 2)
        call.check(norm=R.BONITO)


def test_pod5_python_method():
    c = codec()
    rows, first, frames = frames_of(71, POD5_SHAPES)
    src, off, size = arena(c, frames, 16)
    dev = c.device
    rng = np.random.default_rng(2)
    starts = [pod5_windows(rng, lens, 64) for lens in POD5_SHAPES]
    wfirst = torch.from_numpy(np.concatenate([[0], np.cumsum([len(v) for v in starts])]).astype(np.int64)).to(dev)
    flat = torch.tensor([v for st in starts for v in st], dtype=torch.int32, device=dev)
    res = torch.full((len(rows),), -8, dtype=torch.int32, device=dev)
    rr = torch.full((len(first),), -8, dtype=torch.int32, device=dev)
    out = c.pod5_decompress_windows(src, off, size, i32([len(x) for x in rows]).to(dev), first, res, wfirst, flat, 64, -7.0, torch.float32, read_result=rr)
    torch.cuda.synchronize()
    sig = PR.read_signals(rows, first)
    import windows_ref as W
    want = np.concatenate([W.window_rows(x, None, None, st, 64, 0.0, 1.0, -7.0, "f32") for x, st in zip(sig, starts)])
    assert (out.cpu().numpy().view(np.uint32) == want).all()
    assert u32(rr).tolist() == [4 * len(x) for x in sig] and u32(res).tolist() == [4 * len(x) for x in rows]


# ---- 8. verdicts ------------------------------------------------------------------------------------------------------------------------------------
def verdict_frames(c):
    rng = np.random.default_rng(91)
    return Frames(c, [sine_signal(rng, T) for T in (5000, 3000, 2500, 900)], c.options(True, 2, 1, 1))


def test_window_check_failures_fail_that_read_alone():
    c = codec()
    fr = verdict_frames(c)
    rng = np.random.default_rng(5)
    starts = [random_starts(rng, T, 64, k) for T, k in zip(fr.T, (2, 3, 4, 3))]
    flat = [v for s in starts for v in s]
    for norm in (None, NORMS["med_mad"]):
        # window_first[2] > window_first[3]: the reads own rows 3-4, 5-7, (8 > 0), 0-2
        per = [starts[0], starts[1], [], starts[3]]
        order = starts[3] + starts[0] + starts[1]
        WinRun(fr, per, 64, "f16", first=[3, 5, 8, 0, 3], flat=order, norm=norm).check(expect={2: E_DEST})
        # window_first[4] > window_rows: read 3's rows lie behind the rows the struct declares
        WinRun(fr, starts, 64, "f16", rows=len(flat) - 1, norm=norm).check(expect={3: E_DEST})
        # a decreasing pair inside read 2's rows (and one between two reads' rows, which is none of the check's business)
        bad = [list(s) for s in starts]
        bad[2][2], bad[2][3] = 900, 899
        bad[1][0] = 2990
        bad[1].sort()
        WinRun(fr, bad, 64, "f16", norm=norm).check(expect={2: E_DEST})
    # a long list whose only decreasing pair is its last
    long = [sorted(random_starts(rng, 5000, 16, 3000)), [0], [], [5]]
    long[0][-1] = long[0][-2] - 1
    WinRun(fr, long, 16, "f32").check(expect={0: E_DEST})


def test_a_damaged_frame_keeps_its_verdict():
    c = codec()
    fr = verdict_frames(c)
    src = fr.src.clone()
    size = fr.size.clone()
    size[1] = int(u32(fr.size)[1]) // 2   # the frame of read 1 cut off in its middle
    fr.size = size
    dst = torch.zeros(fr.dst_bytes + 64, dtype=torch.uint8, device=c.device)
    res16 = torch.full((fr.n,), -8, dtype=torch.int32, device=c.device)
    c.decompress(src, fr.off, fr.size, dst, fr.doff, fr.dcap, res16, fr.opts)
    torch.cuda.synchronize()
    un = u32(res16).tolist()
    assert _lib.is_error(un[1]) and not any(_lib.is_error(v) for i, v in enumerate(un) if i != 1), [hex(v) for v in un]
    rng = np.random.default_rng(6)
    starts = [random_starts(rng, T, 64, 5) for T in fr.T]
    WinRun(fr, starts, 64, "f16", src=src).check(expect={1: un[1]}, skip={1})


def test_pod5_verdicts():
    c = codec()
    shapes = [[600, 700], [900, 1000, 1100], [500], [900, 1000, 1100], [640]]
    rows, first, frames = frames_of(21, shapes)
    rng = np.random.default_rng(8)
    starts = [pod5_windows(rng, lens, 64) for lens in shapes]
    b = PR.bounds(first, len(rows))
    sig = PR.read_signals(rows, first)
    # a decreasing pair inside read 1's rows, and read 3's window_first pair the wrong way round
    bad = [list(s) for s in starts]
    bad[1][4], bad[1][5] = bad[1][5] + 1, bad[1][4]
    n4 = len(starts[4])
    flat = bad[0] + bad[1] + starts[4]
    # the same, and: read 2's rows end behind the arena's, read 3's pair is the wrong way round; read 4 owns the last rows
    wfirst = [0, len(bad[0]), len(flat) - n4, len(flat) + 2, len(flat) - n4, len(flat)]
    for which, call, refused in (("sorted", WinCall(c, frames, rows, first, bad, 64, "f16"), {1}),
                                 ("pairs", WinCall(c, frames, rows, first, [bad[0], bad[1], [], [], starts[4]], 64, "f16", wfirst=wfirst, flat=flat), {1, 2, 3})):
        assert call.call() == 0, c.L.vbz_gpu_last_error(c.ctx)
        assert u32(call.result)[: call.n].tolist() == [E_DEST if k in refused else 2 * len(rows[j]) for k in range(len(first)) for j in range(b[k], b[k + 1])], which
        assert u32(call.read_result)[: call.R].tolist() == [E_DEST if k in refused else 2 * len(sig[k]) for k in range(len(first))], which
        call.check(consts=[(0.0, 1.0)] * 5, refused=refused)
    # a bad first_row fails whole
    table = list(b)
    table[0] = 1
    call = WinCall(c, frames, rows, first, starts, 64, "f16", table=table)
    assert call.call() == 0
    assert u32(call.result)[: call.n].tolist() == [E_INPUT] * call.n and u32(call.read_result)[: call.R].tolist() == [E_INPUT] * call.R
    assert (call.out.cpu().numpy() == CANARY).all()
    # a damaged row inside a read: its verdict, the other reads exact
    damaged = list(frames)
    damaged[3] = frames[3][: len(frames[3]) // 2]
    call = WinCall(c, damaged, rows, first, starts, 64, "f16")
    assert call.call() == 0
    res = u32(call.result)[: call.n].tolist()
    assert res[3] == E_ZSTD and [r for j, r in enumerate(res) if j != 3] == [2 * len(x) for j, x in enumerate(rows) if j != 3]
    assert u32(call.read_result)[: call.R].tolist() == [E_ZSTD if k == 1 else 2 * len(sig[k]) for k in range(5)]
    call.check(consts=[(0.0, 1.0)] * 5, skip={1})
