"""Signal events on the MI355X (include/vbz_gpu.h: vbz_gpu_events and the two *_signal_events_batch calls).  Every record and every
moments row is held bit for bit to tests/events_ref.py, result[] beside them, with both arenas filled with a canary and checked outside
the passing reads' rows, guard rows behind them: read lengths around a lane (8 samples), a wavefront (512 is covered by 2 047 ... 2 049),
a tile (2 048) and the paired-tile loop (4 101, 6 151), each as signal-like data, full-range noise and a constant, crossed with the event
lists a caller can give; every option and frame kind; the large-read path, split and routed call shapes; POD5 rows and reads; ranges
and constants."""
import numpy as np
import pytest
import torch

import events_ref as EV
import oracle_lib as O
import pod5_reads_ref as PR
import ranges_ref as G
from events_support import EvCall, EvRun
from typed_support import NORMS, SHAPES, Frames, arena, codec, expect_results, frames_of, i32, sine_signal, u32
from vbz_compression_amd import batch

pytestmark = pytest.mark.gpu

TO_END = 0xFFFFFFFF
LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049, 4101, 6151]


def consts(rng, n):
    o, s = rng.uniform(-600, 600, n).astype(np.float32), rng.uniform(0.01, 2.5, n).astype(np.float32)
    s[::3] *= -1   # (negative scales: sd takes |s|)
    return o, s


def dwell(rng, T, lo=1, hi=30, first=0):
    """starts of events of random dwell lo ... hi samples over a signal of T samples"""
    st, p = [], first
    while p < T:
        st.append(p)
        p += int(rng.integers(lo, hi + 1))
    return st


# the event lists of the issue, for a signal of T samples
LISTS = {
    "none": lambda rng, T: [],
    "zero": lambda rng, T: [0],
    "every_sample": lambda rng, T: list(range(T)),
    "around_lanes": lambda rng, T: sorted({v for k in range(T // 8 + 2) for v in (8 * k - 1, 8 * k, 8 * k + 1) if v >= 0}),
    "around_tiles": lambda rng, T: [v for k in range(1, 4) for v in (2048 * k - 1, 2048 * k + 1)],
    "duplicates": lambda rng, T: sorted([0, 0, 3, 3, 3, T // 2, T // 2, T // 2 + 9] + [max(T - 1, 0)] * 2),
    "at_and_behind_the_end": lambda rng, T: [T // 2, T, T + 1, TO_END],
    "first_start_5": lambda rng, T: dwell(rng, T, 1, 30, 5) or [5],
    "random_dwell": lambda rng, T: dwell(rng, T),
    "mid_lane_over_tiles": lambda rng, T: [3, 3 + 4500, 3 + 4500 + 11],
}


_grid = {}


def grid(c):
    """every length as signal-like data, full-range noise and a constant"""
    if "g" not in _grid:
        rng = np.random.default_rng(17)
        reads = []
        for T in LENGTHS:
            reads += [sine_signal(rng, T), rng.integers(-32768, 32768, T).astype(np.int16), np.full(T, -12345, np.int16)]
        _grid["g"] = Frames(c, reads, c.options(True, 2, 1, 1))
    return _grid["g"]


@pytest.mark.parametrize("kind", list(LISTS))
def test_lengths_and_event_lists(kind):
    c = codec()
    fr = grid(c)
    rng = np.random.default_rng(len(kind))
    o, s = consts(rng, fr.n)
    starts = [LISTS[kind](rng, T) for T in fr.T]
    EvRun(fr, starts, offset=o, scale=s).check()
    EvRun(fr, starts, signed=False, moments=False).check()   # (uint16: the noise and the constant are >= 32768; a NULL moments)


def mixed_starts(rng, T):
    return LISTS[list(LISTS)[int(rng.integers(0, len(LISTS)))]](rng, T)


# ---- options and frame kinds ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sized", [False, True], ids=["unsized", "sized"])
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("version", [0, 1])
@pytest.mark.parametrize("zz", [True, False], ids=["zz", "nozz"])
def test_options(zz, version, level, sized):
    c = codec()
    rng = np.random.default_rng(version * 8 + level * 4 + sized * 2 + zz)
    reads = [sine_signal(rng, T) if (zz and k % 2) else rng.integers(-32768, 32768, T).astype(np.int16) for k, T in enumerate([0, 1, 9, 65, 2049, 4101, 6151, 20_000])]
    fr = Frames(c, reads, c.options(zz, 2, level, version), sized, slack=6)
    o, s = consts(rng, fr.n)
    starts = [dwell(rng, T) for T in fr.T]
    EvRun(fr, starts, offset=o, scale=s).check()
    EvRun(fr, starts, [8, 3] * 4, [TO_END] * 8, norm=NORMS["med_mad"], signed=False).check()


def test_libzstd_frames():
    c = codec()
    rng = np.random.default_rng(51)
    reads = [sine_signal(rng, T) for T in (0, 1, 9, 2049, 4101, 50_000)]
    starts = [mixed_starts(rng, len(x)) for x in reads]
    comp = arena(c, [O.compress(x, O.options(True, 2, 1, 1), sized=True) for x in reads], 64)
    fr = Frames(c, reads, c.options(True, 2, 1, 1), sized=True, comp=comp)
    EvRun(fr, starts, norm=NORMS["med_mad"]).check()
    EvRun(fr, starts, [8] * fr.n, [TO_END] * fr.n, offset=[1.5] * fr.n, scale=[-0.25] * fr.n).check()


# ---- the other decode paths -----------------------------------------------------------------------------------------------------------------
SEG = 16_384


def large_read_checks(c):
    """one read of three segments of the large-read path: events that straddle, begin at and end at the segment edges"""
    rng = np.random.default_rng(23)
    x = sine_signal(rng, 40_000)
    x[:3000] += 3000
    fr = Frames(c, [x], c.options(True, 2, 1, 1))
    edges = sorted({v for k in (1, 2) for v in (k * SEG - 2049, k * SEG - 9, k * SEG - 1, k * SEG, k * SEG + 1, k * SEG + 8)})
    for st in ([3, SEG - 5, 2 * SEG + 100], edges, dwell(rng, 40_000), [5, 39_999, 40_000, TO_END], [7]):
        EvRun(fr, [st], offset=[-37.5], scale=[0.173]).check()
    EvRun(fr, [dwell(rng, SEG + 105)], [SEG - 5], [2 * SEG + 100], norm=NORMS["quantile"], stats=1).check()
    EvRun(fr, [edges], [3], [TO_END], norm=NORMS["med_mad"]).check()


def test_one_large_read_alone_in_a_call():
    large_read_checks(codec())


@pytest.mark.parametrize("segmented", [1, 0])
def test_large_read_on_forced_paths(segmented):
    large_read_checks(codec(VBZ_HIP_SEGMENTED=segmented))


def small_batch(seed, n, lo=50, hi=3000):
    rng = np.random.default_rng(seed)
    reads, starts = [], []
    for i in range(n):
        T = int(rng.integers(lo, hi))
        reads.append(sine_signal(rng, T) if i % 3 else rng.integers(-32768, 32768, T).astype(np.int16))
        starts.append(dwell(rng, T, 1, 200, int(rng.integers(0, 9))))
    return reads, starts


def test_split_batch():
    """the upper half finds its own rows (event_first offset as the other per-read tables)"""
    reads, starts = small_batch(31, 200)
    outs = []
    for c in (codec(VBZ_HIP_SPLIT_MIN=64), codec(VBZ_HIP_SPLIT_MIN=0)):
        fr = Frames(c, reads, c.options(True, 2, 1, 1))
        r = EvRun(fr, starts, norm=NORMS["med_mad"]).check()
        outs.append((r.out.cpu().numpy().tobytes(), r.mom.cpu().numpy().tobytes(), r.ss.cpu().numpy().tobytes()))
        EvRun(fr, starts, moments=False).check()
    assert outs[0] == outs[1]


def test_routed_long_read_among_small_ones():
    c = codec()
    reads, starts = small_batch(41, 600, 500, 5000)
    rng = np.random.default_rng(42)
    reads[100] = sine_signal(rng, 264_000)
    starts[100] = dwell(rng, 264_000, 2, 30, 4)
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    o, s = consts(rng, fr.n)
    EvRun(fr, starts, offset=o, scale=s).check()
    bg, en = [8 if i % 2 else 3 for i in range(fr.n)], [TO_END if i % 3 else 2000 for i in range(fr.n)]
    bg[100], en[100] = 2003, 260_000
    EvRun(fr, starts, bg, en, norm=NORMS["quantile"], stats=1).check()


# ---- ranges and constants ---------------------------------------------------------------------------------------------------------------------
def range_case():
    rng = np.random.default_rng(29)
    reads, bg, en = [], [], []
    for T in (0, 1, 9, 65, 2049, 4101, 6151):
        x = sine_signal(rng, T)
        for b, e in ((0, max(T - 3, 0)), (8, TO_END), (3, max(T - 100, 0)), (8, max(T - 1, 0)), (2048, 2048), (TO_END, 0)):
            reads.append(x)
            bg.append(b)
            en.append(e)
    return reads, bg, en


def test_ranges_with_offset_and_scale_tables():
    c = codec()
    reads, bg, en = range_case()
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    rng = np.random.default_rng(5)
    o, s = consts(rng, fr.n)
    assert (s < 0).any()
    starts = [mixed_starts(rng, G.clamp(T, b, e)[1] - G.clamp(T, b, e)[0]) for T, b, e in zip(fr.T, bg, en)]
    EvRun(fr, starts, bg, en, offset=o, scale=s).check()
    EvRun(fr, starts, bg, None, offset=o).check()
    EvRun(fr, starts, None, en, scale=s).check()


@pytest.mark.parametrize("stats", [0, 1], ids=["range", "read"])
@pytest.mark.parametrize("method", ["med_mad", "quantile"])
def test_normalised_events(method, stats):
    """the constants are the statistics call's shift_scale, bit for bit"""
    c = codec()
    reads, bg, en = range_case()
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    rng = np.random.default_rng(3)
    starts = [dwell(rng, T, 1, 60) for T in fr.T]
    r = EvRun(fr, starts, bg, en, norm=NORMS[method], stats=stats).check()
    res = torch.full((fr.n,), -8, dtype=torch.int32, device=c.device)
    ss = c.signal_norm(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res, fr.opts, NORMS[method][1], begin=bg, end=en, stats=("range", "read")[stats])
    torch.cuda.synchronize()
    assert ss.cpu().numpy().tobytes() == r.ss.cpu().numpy()[: fr.n].tobytes()
    assert u32(res).tolist() == u32(r.result)[: fr.n].tolist()
    EvRun(fr, starts, norm=NORMS[method], stats=stats).check()   # (no ranges: the whole read either way)


# ---- POD5 ---------------------------------------------------------------------------------------------------------------------------------------
def pod5_events(rng, lens, b=0, e=None):
    """events that straddle the row boundaries and the ends of a read's range, over a dwell list"""
    T = sum(lens)
    e = T if e is None else min(e, T)
    b = min(b, e)
    cum = np.cumsum([0] + lens).tolist()
    st = [v - b + k for v in cum for k in (-9, -1, 0, 1, 8) if v - b + k >= 0] + [e - b, e - b + 5, TO_END]
    return sorted(st + dwell(rng, e - b, 1, 300, 2))


@pytest.mark.parametrize("segmented", [0, 1])
def test_pod5_reads(segmented):
    c = codec(VBZ_HIP_SEGMENTED=segmented)
    shapes = SHAPES
    rows, first, frames = frames_of(71, shapes)
    rng = np.random.default_rng(7)
    n = len(first)
    o, s = consts(rng, n)
    starts = [pod5_events(rng, lens) for lens in shapes]
    call = EvCall(c, frames, rows, first, starts, offset=o, scale=s)
    assert call.call() == 0, c.L.vbz_gpu_last_error(c.ctx)
    expect_results(call, rows, first, 2)
    call.check(consts=list(zip(o, s)))
    # every sample its own event, and rows that own nothing
    call = EvCall(c, frames, rows, first, [list(range(sum(lens))) if k % 2 else [] for k, lens in enumerate(shapes)])
    assert call.call() == 0, c.L.vbz_gpu_last_error(c.ctx)
    call.check(consts=[(0.0, 1.0)] * n)
    # ranges: begins at 8 and 3, ends inside and to the end, empty ones
    bg = [8, 3, 8, 3, 0, 8, 3, 2000, 700, TO_END]
    en = [TO_END, 2000, 1000, TO_END, 0, 4000, TO_END, 2100, 20, 0]
    starts = [pod5_events(rng, lens, b, e) for lens, b, e in zip(shapes, bg, en)]
    call = EvCall(c, frames, rows, first, starts, bg, en, offset=o, scale=s)
    assert call.call() == 0, c.L.vbz_gpu_last_error(c.ctx)
    expect_results(call, rows, first, 2)
    call.check(consts=list(zip(o, s)))
    for stats in (0, 1):
        for name in ("med_mad", "quantile"):
            call = EvCall(c, frames, rows, first, starts, bg, en, norm=NORMS[name][1], stats=stats)
            assert call.call() == 0, c.L.vbz_gpu_last_error(c.ctx)
            expect_results(call, rows, first, 2)
            call.check(norm=NORMS[name][0])


def test_python_methods():
    c = codec()
    dev = c.device
    fr = grid(c)
    rng = np.random.default_rng(2)
    starts = [dwell(rng, T) for T in fr.T]
    first = torch.from_numpy(np.concatenate([[0], np.cumsum([len(v) for v in starts])]).astype(np.int64)).to(dev)
    flat = [v for st in starts for v in st]
    res = torch.full((fr.n,), -8, dtype=torch.int32, device=dev)
    mean, sd, n, mom = c.signal_events(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res, fr.opts, first, flat, moments=True)
    torch.cuda.synchronize()
    want = [EV.event_rows(x, None, None, st, 0.0, 1.0) for x, st in zip(fr.reads, starts)]
    rows, moms = np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want])
    assert mean.dtype == torch.float32 and sd.dtype == torch.float32 and n.dtype == torch.int32 and mom.dtype == torch.int64
    assert (mean.cpu().numpy().view(np.uint32) == rows[:, 0]).all() and (sd.cpu().numpy().view(np.uint32) == rows[:, 1]).all()
    assert (n.cpu().numpy().view(np.uint32) == rows[:, 2]).all() and (mom.cpu().numpy() == moms).all()
    assert u32(res).tolist() == [2 * T for T in fr.T]
    assert len(c.signal_events(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res, fr.opts, first, flat, norm=batch.MED_MAD)) == 3
    # POD5
    shapes = [[13, 7, 1, 2047, 2049], [800, 0, 800], [300] * 10, []]
    prow, pfirst, frames = frames_of(71, shapes)
    src, off, size = arena(c, frames, 16)
    starts = [pod5_events(rng, lens) for lens in shapes]
    first = torch.from_numpy(np.concatenate([[0], np.cumsum([len(v) for v in starts])]).astype(np.int64)).to(dev)
    res = torch.full((len(prow),), -8, dtype=torch.int32, device=dev)
    rr = torch.full((len(pfirst),), -8, dtype=torch.int32, device=dev)
    mean, sd, n, mom = c.pod5_signal_events(src, off, size, i32([len(x) for x in prow]).to(dev), pfirst, res, first, [v for st in starts for v in st],
                                            moments=True, read_result=rr)
    torch.cuda.synchronize()
    sig = PR.read_signals(prow, pfirst)
    want = [EV.event_rows(x, None, None, st, 0.0, 1.0) for x, st in zip(sig, starts)]
    rows, moms = np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want])
    assert (mean.cpu().numpy().view(np.uint32) == rows[:, 0]).all() and (sd.cpu().numpy().view(np.uint32) == rows[:, 1]).all()
    assert (n.cpu().numpy().view(np.uint32) == rows[:, 2]).all() and (mom.cpu().numpy() == moms).all()
    assert u32(rr).tolist() == [2 * len(x) for x in sig] and u32(res).tolist() == [2 * len(x) for x in prow]


# ---- the canary ---------------------------------------------------------------------------------------------------------------------------------
def test_rows_of_no_read_stay_untouched():
    """the rows in front of event_first[0] and behind event_first[n] belong to no read: they keep the canary in both arenas, as the guard
    rows do (EvRun.check looks at every row outside the reads' rows)"""
    c = codec()
    rng = np.random.default_rng(61)
    fr = Frames(c, [sine_signal(rng, T) for T in (5000, 3000, 0, 900)], c.options(True, 2, 1, 1))
    starts = [dwell(rng, 5000), dwell(rng, 3000), [0, 4], dwell(rng, 900)]
    first = np.concatenate([[5], 5 + np.cumsum([len(v) for v in starts])]).astype(np.int64)
    flat = [0] * 5 + [v for st in starts for v in st] + [0] * 7
    for moments in (True, False):
        r = EvRun(fr, starts, first=first, flat=flat, offset=[0.5] * 4, scale=[2.0] * 4, moments=moments).check()
        rows = r.out.cpu().numpy().reshape(-1, 16)
        assert (rows[:5] == 0x5A).all() and (rows[int(first[-1]) :] == 0x5A).all() and len(rows) == len(flat) + r.guard
