"""Per-read sample ranges on the MI355X (include/vbz_gpu.h: vbz_gpu_sample_ranges and the *_range_batch calls).  Every case is held bit for
bit to tests/ranges_ref.py -- the clamped range, sliced, as ONE read to the chunking rules and to norm_ref -- with the chunk arena filled
with a canary and checked outside the reads' rows: sizes around a lane (8 samples), a wavefront (512), a tile (2 048) and the paired-tile
loop, crossed with begins and ends at and around them; every output type and option; the large-read path, split and routed call shapes,
libzstd's and checksummed frames; statistics of the range and of the read; POD5 reads of several rows; verdicts and refusals."""
import ctypes

import numpy as np
import pytest
import torch

import norm_ref as R
import oracle_lib as O
import pod5_ref as P
import pod5_reads_ref as PR
import ranges_ref as G
from signal_ref import table_of
from typed_support import (CANARY, ELEM, NORMS, PAD, SHAPES, Call, Frames, Run, arena, codec, expect_results, frames_of, full, i32, ranges_struct, sine_signal,
                           u32, unranged_results)
from vbz_compression_amd import _lib, batch

pytestmark = pytest.mark.gpu

E_ZSTD, E_INPUT, E_DEST, E_STREAM = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFC, 0xFFFFFFFB
TO_END = 0xFFFFFFFF


# ---- 1. small reads: sizes x begins x ends, chunkings x modes -----------------------------------------------------------------------------
SIZES = [0, 1, 7, 8, 9, 511, 513, 2047, 2048, 2049, 4101, 20_000]


def begins_of(T):
    return [0, 1, 7, 8, 9, 2040, 2048, 2051, max(T - 1, 0), T, T + 5, TO_END]


def ends_of(T, b):
    return [0, b, (b + 1) & 0xFFFFFFFF, max(T - 1, 0), T, T + 1, TO_END, b // 2]   # (the last one: end < begin wherever begin > 1)


_grid = {}


def grid(c):
    """every size crossed with every begin and end, a read each: (Frames, begin, end)"""
    if "g" not in _grid:
        rng = np.random.default_rng(17)
        base = {T: (sine_signal(rng, T) if k % 3 else rng.integers(-32768, 32768, T).astype(np.int16)) for k, T in enumerate(SIZES)}
        reads, bg, en = [], [], []
        for T in SIZES:
            for b in begins_of(T):
                for e in ends_of(T, b):
                    reads.append(base[T])
                    bg.append(b)
                    en.append(e)
        _grid["g"] = (Frames(c, reads, c.options(True, 2, 1, 1)), bg, en)
    return _grid["g"]


CHUNKINGS = [(8, 8), (16, 8), (1024, 1000), (4096, 1024)]
MODES = [("pad", 0), ("end", 1), ("end", 6), ("end", 8)]


@pytest.mark.parametrize("mode,ea", MODES, ids=lambda v: str(v))
@pytest.mark.parametrize("L,S", CHUNKINGS)
def test_small_reads_begins_and_ends(L, S, mode, ea):
    c = codec()
    fr, bg, en = grid(c)
    rng = np.random.default_rng(L + ea)
    o, s = rng.uniform(-600, 600, fr.n).astype(np.float32), rng.uniform(0.01, 2.5, fr.n).astype(np.float32)
    Run(fr, (L, S, mode, ea), "f16", bg, en, offset=o, scale=s).check()


@pytest.mark.parametrize("which", ["begin-null", "end-null"])
def test_a_null_table_is_zero_or_the_sample_count(which):
    c = codec()
    fr, bg, en = grid(c)
    for chunking in ((16, 8, "end", 6), (1024, 1000, "pad", 0)):
        Run(fr, chunking, "f16", None if which == "begin-null" else bg, None if which == "end-null" else en).check()


# ---- 2. output types and options ----------------------------------------------------------------------------------------------------------
def option_ranges(T):
    return [(8, T - 3 if T > 3 else T), (3, T), (2048, TO_END), (2051, max(T - 1, 0)), (0, T), (T, T), (16, 17), (2040, 2049)]


@pytest.mark.parametrize("sized", [False, True], ids=["unsized", "sized"])
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("version", [0, 1])
@pytest.mark.parametrize("zz", [True, False], ids=["zz", "nozz"])
def test_output_types_and_options(zz, version, level, sized):
    c = codec()
    rng = np.random.default_rng(version * 8 + level * 4 + sized * 2 + zz)
    reads, bg, en = [], [], []
    for k, T in enumerate([0, 1, 7, 9, 513, 2049, 4101, 20_000]):
        x = sine_signal(rng, T) if (zz and k % 2) else rng.integers(-32768, 32768, T).astype(np.int16)
        for b, e in option_ranges(T):
            reads.append(x)
            bg.append(b)
            en.append(e)
    fr = Frames(c, reads, c.options(zz, 2, level, version), sized, slack=6)
    o, s = rng.uniform(-600, 600, fr.n).astype(np.float32), rng.uniform(0.01, 2.5, fr.n).astype(np.float32)
    for dtype in ("f32", "f16", "bf16"):
        for signed in (True, False):
            Run(fr, (1024, 1000, "end", 6), dtype, bg, en, signed=signed, offset=o, scale=s).check()
    Run(fr, (16, 8, "pad", 0), "f32", bg, en, norm=NORMS["med_mad"], signed=False).check()


# ---- 3. the other decode paths --------------------------------------------------------------------------------------------------------------
SEG = 16_384
LARGE_RANGES = [(SEG - 8, 2 * SEG), (SEG, 2 * SEG + 1), (SEG + 1, 2 * SEG - 1), (SEG - 1, SEG + 1), (8, SEG), (3, SEG + 1), (100, 5000), (104, 5003),
                (2 * SEG, TO_END), (2 * SEG + 1, 40_000), (SEG + 8, SEG + 8), (0, 40_000)]


def large_read_checks(c):
    rng = np.random.default_rng(23)
    x = sine_signal(rng, 40_000)
    x[:3000] += 3000
    fr = Frames(c, [x], c.options(True, 2, 1, 1))
    for k, (b, e) in enumerate(LARGE_RANGES):
        chunking = [(4096, 1024, "end", 6), (1024, 1000, "pad", 0), (16, 8, "end", 1)][k % 3]
        Run(fr, chunking, ["f16", "f32", "bf16"][k % 3], [b], [e], offset=[-37.5], scale=[0.173]).check()
        Run(fr, chunking, "f16", [b], [e], norm=NORMS["med_mad" if k % 2 else "quantile"], stats=k % 4 // 2).check()
        stats_alone(fr, [b], [e], NORMS["quantile" if k % 2 else "med_mad"])


def test_one_large_read_alone_in_a_call():
    large_read_checks(codec())


@pytest.mark.parametrize("segmented", [1, 0])
def test_large_read_on_forced_paths(segmented):
    large_read_checks(codec(VBZ_HIP_SEGMENTED=segmented))


def small_batch(seed, n, lo=50, hi=3000):
    rng = np.random.default_rng(seed)
    reads, bg, en = [], [], []
    for i in range(n):
        T = int(rng.integers(lo, hi))
        reads.append(sine_signal(rng, T) if i % 3 else rng.integers(-32768, 32768, T).astype(np.int16))
        b = int(rng.integers(0, T + 20))
        bg.append(b & ~7 if i % 2 else b)   # (every other begin a multiple of 8)
        en.append(int(rng.integers(0, T + 20)) if i % 5 else TO_END)
    return reads, bg, en


def test_split_batch():
    reads, bg, en = small_batch(31, 200)
    outs = []
    for c in (codec(VBZ_HIP_SPLIT_MIN=64), codec(VBZ_HIP_SPLIT_MIN=0)):
        fr = Frames(c, reads, c.options(True, 2, 1, 1))
        r = Run(fr, (1024, 1000, "end", 6), "f16", bg, en, norm=NORMS["med_mad"]).check()
        outs.append((r.chunks.cpu().numpy().tobytes(), r.ss.cpu().numpy().tobytes()))
        Run(fr, (16, 8, "pad", 0), "bf16", bg, en).check()
        stats_alone(fr, bg, en, NORMS["quantile"])
    assert outs[0] == outs[1]


def test_routed_long_read_among_small_ones():
    c = codec()
    reads, bg, en = small_batch(41, 600, 500, 5000)
    rng = np.random.default_rng(42)
    for i, (T, b, e) in {100: (300_000, 2000, 298_000), 400: (300_000, 2003, TO_END), 500: (280_001, SEG + 1, 3 * SEG)}.items():
        reads[i] = sine_signal(rng, T)
        reads[i][:b] += 3000
        bg[i], en[i] = b, e
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    Run(fr, (10_000, 9504, "end", 1), "f16", bg, en, norm=NORMS["med_mad"]).check()
    Run(fr, (4096, 1024, "pad", 0), "f32", bg, en, norm=NORMS["quantile"], stats=1).check()
    stats_alone(fr, bg, en, NORMS["med_mad"])


def other_frames_reads():
    rng = np.random.default_rng(51)
    reads, bg, en = [], [], []
    for T in (0, 1, 9, 2049, 4101, 50_000):
        for b, e in ((8, T), (3, max(T - 5, 0)), (2048, TO_END), (2051, T + 1)):
            reads.append(sine_signal(rng, T))
            bg.append(b)
            en.append(e)
    return reads, bg, en


def test_libzstd_frames():
    c = codec()
    reads, bg, en = other_frames_reads()
    comp = arena(c, [O.compress(x, O.options(True, 2, 1, 1), sized=True) for x in reads], 64)
    fr = Frames(c, reads, c.options(True, 2, 1, 1), sized=True, comp=comp)
    Run(fr, (1024, 1000, "end", 6), "f16", bg, en, norm=NORMS["med_mad"]).check()
    Run(fr, (16, 8, "pad", 0), "f32", bg, en).check()


def test_checksummed_frames():
    c = codec()
    reads, bg, en = other_frames_reads()
    c.set_checksum(1)
    try:
        fr = Frames(c, reads, c.options(True, 2, 1, 1))
    finally:
        c.set_checksum(0)
    Run(fr, (1024, 1000, "end", 8), "bf16", bg, en, norm=NORMS["quantile"]).check()
    Run(fr, (4096, 1024, "pad", 0), "f16", bg, en).check()


# ---- 4. statistics --------------------------------------------------------------------------------------------------------------------------
def stats_alone(fr, begin, end, norm, signed=True, stats=0):
    """vbz_gpu_signal_norm_range_batch against ranges_ref; result[i] the int16 decode's"""
    c = fr.c
    res = torch.full((max(fr.n, 1),), -8, dtype=torch.int32, device=c.device)
    ss = c.signal_norm(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res, fr.opts, norm[1], signed=signed, sized=fr.sized, begin=begin, end=end,
                       stats={0: "range", 1: "read"}[stats])
    torch.cuda.synchronize()
    ss = ss.cpu().numpy()
    bg, en = full(begin, fr.n), full(end, fr.n)
    assert u32(res)[: fr.n].tolist() == [2 * t for t in fr.T]
    for i, x in enumerate(fr.reads):
        shift, scale, _, _ = G.shift_scale(x if signed else x.view(np.uint16), bg[i], en[i], norm[0], stats)
        assert (ss[i][0].view(np.uint32), ss[i][1].view(np.uint32)) == (shift.view(np.uint32), scale.view(np.uint32)), (
            i, fr.T[i], bg[i], en[i], ss[i], shift, scale)
    return ss


def stats_reads():
    rng = np.random.default_rng(61)
    reads, bg, en = [], [], []
    for T, b in ((9000, 2000), (9001, 2003), (2049, 8), (513, 100)):
        x = sine_signal(rng, T) - 330      # the first `begin` samples at +3 000, the rest around 0
        x[:b] += 3000
        reads.append(x.astype(np.int16))
        bg.append(b)
        en.append(TO_END)
        y = (rng.normal(-20_000, 300, T)).astype(np.int16)   # the first sample far from the range's values: outside the anchored windows
        y[:b] = 20_000
        reads.append(y)
        bg.append(b)
        en.append(T - 1)
        reads.append(rng.integers(-32768, 32768, T).astype(np.int16))   # full-range noise
        bg.append(b + 1)
        en.append(T - 7)
    for Tp in (0, 1, 2):   # ranges of 0, 1 and 2 samples, at an aligned and at an odd begin
        for b in (16, 21):
            reads.append(sine_signal(rng, 700))
            bg.append(b)
            en.append(b + Tp)
    return reads, bg, en


@pytest.mark.parametrize("method", ["med_mad", "quantile"])
def test_statistics_of_the_range_and_of_the_read(method):
    c = codec()
    reads, bg, en = stats_reads()
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    by_range = stats_alone(fr, bg, en, NORMS[method])
    by_read = stats_alone(fr, bg, en, NORMS[method], stats=1)
    assert by_range[0].tobytes() != by_read[0].tobytes(), "the trimmed start must move the statistics"
    assert by_range[1].tobytes() != by_read[1].tobytes()
    stats_alone(fr, bg, en, NORMS[method], signed=False)
    for stats in (0, 1):
        r = Run(fr, (1024, 1000, "end", 6), "f16", bg, en, norm=NORMS[method], stats=stats).check()
        ss = r.ss.cpu().numpy()[: fr.n]
        assert ss.tobytes() == (by_range if stats == 0 else by_read).tobytes()


# ---- 5. POD5 reads of several rows -------------------------------------------------------------------------------------------------------
POD5_SHAPES = [[13, 7, 1, 2047, 2049], [800, 0, 800], [24, 8, 2056, 16], [300] * 40, []]


def pod5_ranges(lens):
    """ranges of a read with the given row lengths"""
    T = sum(lens)
    cum = np.cumsum([0] + lens).tolist()
    nz = [k for k, n in enumerate(lens) if n]
    out = [(0, T), (0, TO_END), (T, T), (TO_END, 0)]           # everything; everything left out
    if nz:
        k0, k1 = nz[0], nz[-1]
        out += [(cum[k0] + max(lens[k0] // 2, 1) - 1 if lens[k0] > 1 else cum[k0], T),   # begin inside a row
                (cum[min(k0 + 1, len(lens) - 1)], T),                                    # begin on a row boundary
                (0, cum[k1] + (lens[k1] + 1) // 2),                                      # end inside the last row
                (3, cum[k1] + (lens[k1] + 1) // 2),
                (8, max(T - 8, 0))]
        if len(nz) >= 3:
            out += [(cum[nz[1]], cum[nz[-1]]), (cum[nz[1]] + 5, cum[nz[-1]] - 3), (cum[nz[1]] + 8, TO_END)]   # whole rows left out at either end
    return out


def pod5_case(shapes=POD5_SHAPES):
    all_shapes, bg, en = [], [], []
    for lens in shapes:
        for b, e in pod5_ranges(lens):
            all_shapes.append(lens)
            bg.append(b)
            en.append(e)
    rows, first, frames = frames_of(71, all_shapes)
    return rows, first, frames, bg, en


class RangedCall(Call):
    """Call with the reads' ranges: chunk_first is the layout of the ranges' sample counts"""

    def __init__(self, c, frames, rows, first, begin, end, dtype="f16", chunking=None, norm=None, stats=0, chunk_first=None, **kw):
        table = PR.bounds(first, len(rows))
        self.sig = G.pod5_signals(rows, first)
        self.bg, self.en = full(begin, len(first)), full(end, len(first))
        self.Tp = [e - b for b, e in (G.clamp(len(x), self.bg[k], self.en[k]) for k, x in enumerate(self.sig))]
        if chunking is not None and chunk_first is None:
            chunk_first = table_of(self.Tp, *chunking)
        super().__init__(c, frames, [len(x) for x in rows], table, dtype, chunking, norm=norm, chunk_first=chunk_first, **kw)
        if chunking is not None:
            self.rows = int(max(self.first_host))
        self.g, self.gkeep = ranges_struct(c, begin, end, stats)
        self.stats = stats

    def chunk_call(self):
        m = ctypes.byref(self.m) if self.m is not None else None
        rc = self.c.L.vbz_gpu_pod5_decompress_chunks_range_batch(self.c.ctx, ctypes.byref(self.b), ctypes.byref(self.opts), ctypes.byref(self.f),
                                                                 ctypes.byref(self.ch), ctypes.byref(self.reads), self.chunk_first.data_ptr(),
                                                                 self.chunks.data_ptr(), self.rows, m, self.ss.data_ptr() if self.m is not None else None,
                                                                 ctypes.byref(self.g))
        self.c.synchronize()
        return rc

    def stats_call(self, signed=True):
        rc = self.c.L.vbz_gpu_pod5_signal_norm_range_batch(self.c.ctx, ctypes.byref(self.b), ctypes.byref(self.opts), int(signed), ctypes.byref(self.reads),
                                                           ctypes.byref(self.m), self.ss.data_ptr(), ctypes.byref(self.g))
        self.c.synchronize()
        return rc

    def check_chunks(self, chunking, norm=None, consts=None, skip=()):
        L, S, mode, ea = chunking
        got = self.chunk_bits()
        cf = self.first_host
        ss = self.ss.cpu().numpy()
        for k, x in enumerate(self.sig):
            if k in skip:
                continue
            if norm is not None:
                starts, want, shift, scale = G.norm_chunk_rows(x, self.bg[k], self.en[k], L, S, mode, ea, norm, self.stats, PAD, self.dtype)
                assert (ss[k][0].view(np.uint32), ss[k][1].view(np.uint32)) == (shift.view(np.uint32), scale.view(np.uint32)), ("shift_scale", k)
            else:
                starts, want = G.chunk_rows(x, self.bg[k], self.en[k], L, S, mode, ea, consts[k][0], consts[k][1], PAD, self.dtype)
            assert cf[k + 1] - cf[k] == len(starts), k
            bad = np.argwhere(got[cf[k] : cf[k + 1]] != want)
            assert bad.size == 0, (chunking, self.dtype, "read", k, "range", self.bg[k], self.en[k], "chunk, position", bad[:4].tolist())
        assert (self.chunks.cpu().numpy()[self.rows * L * ELEM[self.dtype] :] == CANARY).all(), "rows behind chunk_first[n] were written"

    def check_stats(self, norm, signed=True):
        ss = self.ss.cpu().numpy()
        for k, x in enumerate(self.sig):
            shift, scale, _, _ = G.shift_scale(x if signed else x.view(np.uint16), self.bg[k], self.en[k], norm, self.stats)
            assert (ss[k][0].view(np.uint32), ss[k][1].view(np.uint32)) == (shift.view(np.uint32), scale.view(np.uint32)), (k, len(x), self.bg[k], self.en[k])


@pytest.mark.parametrize("segmented", [0, 1])
@pytest.mark.parametrize("chunking", [(8, 8, "pad", 0), (16, 8, "end", 1), (1024, 1000, "end", 6), (1024, 1000, "end", 8), (4096, 1024, "pad", 0)],
                         ids=lambda c: "L%d-S%d-%s%d" % c)
def test_pod5_reads(segmented, chunking):
    c = codec(VBZ_HIP_SEGMENTED=segmented)
    rows, first, frames, bg, en = pod5_case()
    rng = np.random.default_rng(5)
    o, s = rng.uniform(-600, 600, len(first)).astype(np.float32), rng.uniform(0.01, 2.5, len(first)).astype(np.float32)
    want = unranged_results(c, frames, rows, first, chunking)
    for dtype in (("f32", "f16", "bf16") if chunking[3] == 6 else ("f16",)):
        call = RangedCall(c, frames, rows, first, bg, en, dtype, chunking, offset=o, scale=s)
        assert call.chunk_call() == 0, c.L.vbz_gpu_last_error(c.ctx)
        expect_results(call, rows, first, ELEM[dtype])
        if dtype == "f16":
            assert (u32(call.result)[: call.n].tolist(), u32(call.read_result)[: call.R].tolist()) == want
        call.check_chunks(chunking, consts=list(zip(o, s)))


@pytest.mark.parametrize("segmented", [0, 1])
def test_pod5_reads_statistics(segmented):
    c = codec(VBZ_HIP_SEGMENTED=segmented)
    rows, first, frames, bg, en = pod5_case()
    chunking = (1024, 1000, "end", 6)
    for name, (p, nm) in NORMS.items():
        want = unranged_results(c, frames, rows, first, None, nm)
        for stats in (0, 1):
            call = RangedCall(c, frames, rows, first, bg, en, norm=nm, stats=stats)
            assert call.stats_call() == 0
            assert (u32(call.result)[: call.n].tolist(), u32(call.read_result)[: call.R].tolist()) == want
            call.check_stats(p)
            call = RangedCall(c, frames, rows, first, bg, en, "f16", chunking, norm=nm, stats=stats)
            assert call.chunk_call() == 0
            expect_results(call, rows, first, 2)
            call.check_chunks(chunking, norm=p)
    call = RangedCall(c, frames, rows, first, bg, en, norm=batch.MED_MAD, signed=False)
    assert call.stats_call(signed=False) == 0
    call.check_stats(R.BONITO, signed=False)


def test_pod5_reads_split_shape():
    rng = np.random.default_rng(81)
    shapes = [[int(v) for v in rng.integers(0, 900, int(rng.integers(1, 6)))] for _ in range(70)]
    rows, first, frames = frames_of(81, shapes)
    bg, en = [], []
    for k, lens in enumerate(shapes):
        T = sum(lens)
        b = int(rng.integers(0, T + 10))
        bg.append(b & ~7 if k % 2 else b)
        en.append(int(rng.integers(0, T + 10)) if k % 4 else TO_END)
    chunking = (1024, 1000, "end", 6)
    outs = []
    for c in (codec(VBZ_HIP_SPLIT_MIN=64), codec(VBZ_HIP_SPLIT_MIN=0)):
        call = RangedCall(c, frames, rows, first, bg, en, "f16", chunking, norm=batch.MED_MAD)
        assert call.chunk_call() == 0
        expect_results(call, rows, first, 2)
        call.check_chunks(chunking, norm=R.BONITO)
        outs.append((call.chunks.cpu().numpy().tobytes(), call.ss.cpu().numpy().tobytes()))
    assert outs[0] == outs[1]


def test_pod5_rows_as_reads_of_their_own():
    """the row-wise calls with POD5 options (a row counts as a read): the svb16 decoder's ranged stores and counting pass"""
    c = codec()
    lens = [0, 1, 7, 9, 513, 2047, 2049, 4101, 20_000]
    rows, first, frames = frames_of(73, [[n] for n in lens for _ in range(6)])
    bg, en = [], []
    for n in lens:
        for b, e in ((8, n), (3, max(n - 5, 0)), (2048, TO_END), (2051, n + 1), (0, n), (n, 0)):
            bg.append(b)
            en.append(e)
    fr = Frames(c, rows, batch.pod5_options(), comp=arena(c, frames, 64))
    Run(fr, (1024, 1000, "end", 6), "f16", bg, en, norm=NORMS["med_mad"]).check()
    Run(fr, (16, 8, "pad", 0), "f32", bg, en, norm=NORMS["quantile"], stats=1).check()
    Run(fr, (4096, 1024, "end", 1), "bf16", bg, en, offset=np.full(fr.n, -37.5, np.float32), scale=np.full(fr.n, 0.173, np.float32)).check()
    stats_alone(fr, bg, en, NORMS["quantile"])


# ---- 6. verdicts ------------------------------------------------------------------------------------------------------------------------------
def test_chunk_first_of_the_whole_read_is_refused():
    c = codec()
    rng = np.random.default_rng(91)
    reads = [sine_signal(rng, T) for T in (5000, 3000, 2500, 900)]
    bg, en = [0, 2000, 8, 100], [5000, TO_END, 1500, 200]   # K(T') != K(T) for reads 1 and 2; read 3 has one chunk either way
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    chunking = (1024, 1000, "pad", 0)
    whole = table_of(fr.T, *chunking)
    r = Run(fr, chunking, "f16", bg, en, chunk_first=whole)
    r.check(expect={1: E_DEST, 2: E_DEST})
    got = r.chunks.cpu().numpy().reshape(-1, 1024 * 2)
    assert (got[whole[1] : whole[3]] == CANARY).all(), "a read that failed the chunk check was written"
    r = Run(fr, chunking, "f16", bg, en, chunk_first=whole, norm=NORMS["med_mad"])
    r.check(expect={1: E_DEST, 2: E_DEST})
    assert (r.chunks.cpu().numpy().reshape(-1, 1024 * 2)[whole[1] : whole[3]] == CANARY).all()


def test_damage_behind_the_end_keeps_its_verdict():
    c = codec()
    rng = np.random.default_rng(92)
    reads = [sine_signal(rng, 9000) for _ in range(6)]
    opts = c.options(True, 2, 0, 1)   # (level 0: the svb stream itself, so the damage is the stream's)
    fr = Frames(c, reads, opts)
    src = fr.src.clone()
    offs, sizes = fr.off.cpu().numpy(), u32(fr.size)
    src[int(offs[1]) + int(sizes[1]) - 40 : int(offs[1]) + int(sizes[1]) - 36] = 0xFF   # data bytes of the last samples: values change, lengths hold
    size = fr.size.clone()
    size[3] = int(sizes[3]) - 5                                                         # a stream cut short behind the range
    src[int(offs[4]) + 9000 // 4 - 3] = 0xFF                                            # control bytes of the last samples announce more bytes
    fr.size = size
    bg, en = [0, 8, 3, 16, 5, 0], [9000, 4000, 4001, 4000, 4000, 100]
    dst = torch.zeros(fr.dst_bytes + 64, dtype=torch.uint8, device=c.device)
    res16 = torch.full((fr.n,), -8, dtype=torch.int32, device=c.device)
    c.decompress(src, fr.off, fr.size, dst, fr.doff, fr.dcap, res16, opts)
    torch.cuda.synchronize()
    un = u32(res16).tolist()
    assert un[3] == E_STREAM and _lib.is_error(un[4]) and un[1] == 18_000
    expect = {i: v for i, v in enumerate(un) if _lib.is_error(v)}   # (their rows are unspecified: skipped, not held to the canary)
    Run(fr, (1024, 1000, "pad", 0), "f16", bg, en, src=src).check(expect=expect, skip=set(expect))
    Run(fr, (1024, 1000, "pad", 0), "f16", bg, en, src=src, norm=NORMS["med_mad"]).check(expect=expect, skip=set(expect))
    res = torch.full((fr.n,), -8, dtype=torch.int32, device=c.device)
    c.signal_norm(src, fr.off, fr.size, fr.doff, fr.dcap, res, opts, batch.MED_MAD, begin=bg, end=en)
    torch.cuda.synchronize()
    assert u32(res).tolist() == un
    # a zstd frame damaged in its middle: whatever the un-ranged decode says of it
    fr2 = Frames(c, reads[:3], c.options(True, 2, 1, 1))
    src2 = fr2.src.clone()
    o2, s2 = fr2.off.cpu().numpy(), u32(fr2.size)
    src2[int(o2[1]) + int(s2[1]) // 2 : int(o2[1]) + int(s2[1]) // 2 + 4] ^= 0x5A
    res16 = torch.full((3,), -8, dtype=torch.int32, device=c.device)
    c.decompress(src2, fr2.off, fr2.size, dst, fr2.doff, fr2.dcap, res16, fr2.opts)
    torch.cuda.synchronize()
    un2 = u32(res16).tolist()
    Run(fr2, (1024, 1000, "pad", 0), "f16", [0, 8, 3], [9000, 100, 4001], src=src2).check(expect={1: un2[1]} if _lib.is_error(un2[1]) else None, skip={1})


def test_pod5_row_failing_inside_a_read():
    c = codec()
    shapes = [[600, 700], [900, 1000, 1100], [500], [900, 1000, 1100], [640]]
    rows, first, good = frames_of(21, shapes)
    frames = list(good)
    frames[3] = good[3][: len(good[3]) // 2]                       # a damaged frame in the middle row of read 1
    frames[7] = O.zstd_compress(P.svb16_encode(rows[7])[:-1], 1)   # a stream with a byte cut off in the middle row of read 3
    chunking = (1024, 1000, "pad", 0)
    bg, en = [8, 100, 3, 0, 600], [1000, 800, TO_END, 850, 700]    # (the failing rows lie behind the ranges of reads 1 and 3)
    want = unranged_results(c, frames, rows, first, chunking, batch.MED_MAD)
    assert want[0][3] == E_ZSTD and want[0][7] == E_STREAM
    call = RangedCall(c, frames, rows, first, bg, en, "f16", chunking, norm=batch.MED_MAD)
    assert call.chunk_call() == 0
    assert (u32(call.result)[: call.n].tolist(), u32(call.read_result)[: call.R].tolist()) == want
    call.check_chunks(chunking, norm=R.BONITO, skip=(1, 3))
    # a POD5 read whose chunk_first is the whole read's
    sig = G.pod5_signals(rows, first)
    whole = table_of([len(x) for x in sig], *chunking)
    call = RangedCall(c, good, rows, first, bg, en, "f16", chunking, chunk_first=whole)
    assert call.chunk_call() == 0
    ok = [len(PR.chunk_starts(t, 1024, 1000, "pad", 0)) == int(whole[k + 1] - whole[k]) for k, t in enumerate(call.Tp)]
    assert ok == [False, False, True, False, True]
    refused = [k for k in range(5) if not ok[k]]
    b = PR.bounds(first, len(rows))
    assert u32(call.result)[: call.n].tolist() == [2 * len(rows[j]) if ok[k] else E_DEST for k in range(len(first)) for j in range(b[k], b[k + 1])]
    assert u32(call.read_result)[: call.R].tolist() == [2 * len(sig[k]) if ok[k] else E_DEST for k in range(len(first))]
    got = call.chunks.cpu().numpy().reshape(-1, 1024 * 2)
    for k in refused:
        assert (got[whole[k] : whole[k + 1]] == CANARY).all(), "a read that failed the chunk check was written"
    call.check_chunks(chunking, consts=[(0.0, 1.0)] * 5, skip=refused)


def test_host_refusals_launch_nothing():
    c = codec()
    L = c.L
    rng = np.random.default_rng(93)
    reads = [sine_signal(rng, 500) for _ in range(4)]
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    n = fr.n
    res = torch.full((n,), 12345, dtype=torch.int32, device=c.device)
    ss = torch.full((n, 2), 7.0, dtype=torch.float32, device=c.device)
    chunks = torch.full((8, 1024), 3.0, dtype=torch.float16, device=c.device)
    first = torch.arange(n + 1, dtype=torch.int64, device=c.device)
    samples = i32(fr.T).to(c.device)
    out = torch.full((n,), 777, dtype=torch.int32, device=c.device)
    b = c._batch(fr.src, fr.off, fr.size, torch.empty(0, dtype=torch.uint8, device=c.device), fr.doff, fr.dcap, res)
    b.dst, b.dst_bytes = None, fr.dst_bytes
    f = _lib.GpuSignalFormat()
    f.out_type, f.is_signed = _lib.VBZ_GPU_SIGNAL_F16, 1
    ch = c._chunking(1024, 1000, "pad", 0)
    m = batch.MED_MAD.c_struct()
    rows, rfirst, frames = frames_of(22, [[600, 700], [900, 1000, 1100], [500, 20]])
    pc = Call(c, frames, [len(x) for x in rows], PR.bounds(rfirst, len(rows)), "f16", (1024, 1000, "pad", 0), norm=batch.MED_MAD)

    def calls(g, which=range(5), o=fr.opts, fmt=f, chk=ch, mp=m):
        gp = ctypes.byref(g)
        fns = [
            lambda: L.vbz_gpu_range_samples_batch(c.ctx, n, samples.data_ptr(), gp, out.data_ptr()),
            lambda: L.vbz_gpu_decompress_chunks_range_batch(c.ctx, ctypes.byref(b), ctypes.byref(o), 0, ctypes.byref(fmt), ctypes.byref(chk),
                                                            first.data_ptr(), chunks.data_ptr(), 8, ctypes.byref(mp), ss.data_ptr(), gp),
            lambda: L.vbz_gpu_signal_norm_range_batch(c.ctx, ctypes.byref(b), ctypes.byref(o), 0, 1, ctypes.byref(mp), ss.data_ptr(), gp),
            lambda: L.vbz_gpu_pod5_decompress_chunks_range_batch(c.ctx, ctypes.byref(pc.b), ctypes.byref(pc.opts), ctypes.byref(pc.f), ctypes.byref(pc.ch),
                                                                 ctypes.byref(pc.reads), pc.chunk_first.data_ptr(), pc.chunks.data_ptr(), pc.rows,
                                                                 ctypes.byref(pc.m), pc.ss.data_ptr(), gp),
            lambda: L.vbz_gpu_pod5_signal_norm_range_batch(c.ctx, ctypes.byref(pc.b), ctypes.byref(pc.opts), 1, ctypes.byref(pc.reads), ctypes.byref(pc.m),
                                                           pc.ss.data_ptr(), gp),
        ]
        return [fns[k]() for k in which]

    bg = [0] * 3
    for kw in ({"reserved": 1}, {"stats": 2}, {"stats": 0xFFFFFFFF}):
        g, keep = ranges_struct(c, bg + [0], None, **kw)
        assert calls(g) == [-2] * 5, kw
        assert L.vbz_gpu_last_error(c.ctx).decode() != ""
    # what the counterparts refuse: unknown options, a bad chunking, a bad normalisation, a format with constants beside norm
    g, keep = ranges_struct(c, bg + [0], None)
    assert calls(g, (1, 2), o=_lib.CompressionOptions(True, 4, 1, 1)) == [-2, -2]
    assert calls(g, (1,), chk=c._chunking(1020, 1000, "pad", 0)) == [-2]
    bad_m = batch.MED_MAD.c_struct()
    bad_m.method = 9
    assert calls(g, (1, 2), mp=bad_m) == [-2, -2]
    scale = torch.ones(n, dtype=torch.float32, device=c.device)
    f2 = _lib.GpuSignalFormat()
    f2.out_type, f2.is_signed, f2.scale = _lib.VBZ_GPU_SIGNAL_F16, 1, scale.data_ptr()
    assert calls(g, (1,), fmt=f2) == [-2]
    assert L.vbz_gpu_range_samples_batch(c.ctx, n, None, ctypes.byref(g), out.data_ptr()) == -2
    assert L.vbz_gpu_signal_norm_range_batch(c.ctx, ctypes.byref(b), ctypes.byref(fr.opts), 0, 1, ctypes.byref(m), None, ctypes.byref(g)) == -2
    assert L.vbz_gpu_decompress_chunks_range_batch(None, ctypes.byref(b), ctypes.byref(fr.opts), 0, ctypes.byref(f), ctypes.byref(ch), first.data_ptr(),
                                                   chunks.data_ptr(), 8, None, None, ctypes.byref(g)) == -1
    torch.cuda.synchronize()
    assert (res.cpu() == 12345).all() and (ss.cpu() == 7.0).all() and (chunks.cpu() == 3.0).all() and (out.cpu() == 777).all()
    assert (pc.chunks.cpu().numpy() == CANARY).all() and (pc.ss.cpu().numpy() == -777.0).all() and (pc.result.cpu() == -8).all()


# ---- 7. the layout call and the un-ranged calls ---------------------------------------------------------------------------------------------
def test_range_samples_feeds_the_layout():
    c = codec()
    Ts = [0, 1, 9, 5000, 0x80000000, 0xFFFFFFFC, 100_003, 7]
    bg = [0, 1, 3, 2000, 5, 0, TO_END, 2]
    en = [5, 0, TO_END, 4999, 9, 0, TO_END, 100]
    samples = i32(Ts).to(c.device)
    for b, e in ((bg, en), (None, en), (bg, None), (None, None)):
        got = c.range_samples(samples, begin=b, end=e)
        torch.cuda.synchronize()
        want = G.range_samples(Ts, b, e)
        assert u32(got).tolist() == want
        first, info = c.chunk_layout(got, 1024, 1000, mode="end", end_align=6)
        torch.cuda.synchronize()
        Tr = [t if t < 0x80000000 else 0 for t in want]
        assert first.cpu().numpy().tolist() == table_of(Tr, 1024, 1000, "end", 6).tolist()
        assert info.cpu().numpy().tolist() == [[i, int(s)] for i, t in enumerate(Tr) for s in PR.chunk_starts(t, 1024, 1000, "end", 6)]


def test_no_ranges_and_whole_ranges_are_the_existing_calls():
    c = codec()
    reads, _, _ = small_batch(95, 120, 0, 6000)
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    samples = i32(fr.T).to(c.device)
    n = fr.n
    for norm in (None, batch.MED_MAD):
        outs = []
        for kw in ({}, {"begin": [0] * n, "end": fr.T}, {"begin": [0] * n}, {"end": [TO_END] * n}, {"begin": [0] * n, "end": fr.T, "stats": "read"}):
            if "stats" in kw and norm is None:
                continue
            res = torch.full((n,), -8, dtype=torch.int32, device=c.device)
            ss = torch.full((n, 2), -777.0, dtype=torch.float32, device=c.device)
            ch, cf, info = c.decompress_chunks(fr.src, fr.off, fr.size, samples, res, fr.opts, 1024, 1000, mode="end", end_align=6, pad=PAD, norm=norm,
                                               norm_out=ss if norm is not None else None, **kw)
            torch.cuda.synchronize()
            outs.append((ch.view(torch.int16).cpu().numpy().tobytes(), cf.cpu().numpy().tobytes(), info.cpu().numpy().tobytes(), u32(res).tolist(),
                         ss.cpu().numpy().tobytes()))
        assert all(o == outs[0] for o in outs[1:])
        # ranges == NULL through the new entry point
        r = Run(fr, (1024, 1000, "end", 6), "f16", norm=(R.BONITO, norm) if norm is not None else None, ranges=False)
        assert r.rc == 0 and r.chunks.cpu().numpy()[: len(outs[0][0])].tobytes() == outs[0][0] and u32(r.result).tolist() == outs[0][3]
    # the POD5 calls
    rows, first, frames = frames_of(1, SHAPES)
    src, off, size = arena(c, frames, 16)
    rs = i32([len(x) for x in rows]).to(c.device)
    sig = G.pod5_signals(rows, first)
    outs = []
    for kw in ({}, {"begin": [0] * len(first), "end": [len(x) for x in sig]}):
        res = torch.full((len(rows),), -8, dtype=torch.int32, device=c.device)
        ss = torch.full((len(first), 2), -777.0, dtype=torch.float32, device=c.device)
        ch, cf, info, rr = c.pod5_decompress_chunks(src, off, size, rs, first, res, 1024, 1000, mode="end", end_align=6, pad=PAD, norm=batch.MED_MAD,
                                                    norm_out=ss, **kw)
        res2 = torch.full((len(rows),), -8, dtype=torch.int32, device=c.device)
        ss2, rr2 = c.pod5_signal_norm(src, off, size, rs, first, res2, batch.DORADO_QUANTILE, **kw)
        torch.cuda.synchronize()
        outs.append((ch.view(torch.int16).cpu().numpy().tobytes(), cf.cpu().numpy().tobytes(), info.cpu().numpy().tobytes(), u32(res).tolist(),
                     u32(rr).tolist(), ss.cpu().numpy().tobytes(), ss2.cpu().numpy().tobytes(), u32(res2).tolist(), u32(rr2).tolist()))
    assert outs[0] == outs[1]


def test_packed_chunks_with_ranges():
    c = codec()
    reads, bg, en = small_batch(97, 60, 0, 5000)
    fr = Frames(c, reads, c.options(True, 2, 1, 1), sized=True)
    packed, poff, psize = c.pack(fr.src, fr.off, c_caps(fr), fr.size, align=16)
    ss = torch.full((fr.n, 2), -777.0, dtype=torch.float32, device=c.device)
    ch, cf, info, res = c.decompress_packed_chunks(packed, poff, psize, fr.opts, 1024, 1000, mode="end", end_align=6, pad=PAD, norm=batch.MED_MAD,
                                                   norm_out=ss, begin=bg, end=en)
    torch.cuda.synchronize()
    assert u32(res).tolist() == [2 * t for t in fr.T]
    cf = cf.cpu().numpy()
    got = ch.view(torch.int16).cpu().numpy().view(np.uint16)
    want_info = []
    for i, x in enumerate(fr.reads):
        starts, want, shift, scale = G.norm_chunk_rows(x, bg[i], en[i], 1024, 1000, "end", 6, R.BONITO, 0, PAD, "f16")
        assert cf[i + 1] - cf[i] == len(starts) and (got[cf[i] : cf[i + 1]] == want).all(), i
        want_info += [[i, int(s)] for s in starts]
    assert info.cpu().numpy().tolist() == want_info


def c_caps(fr):
    return i32([fr.c.L.vbz_max_compressed_size(int(a.nbytes), ctypes.byref(fr.opts)) for a in fr.reads]).to(fr.c.device)
