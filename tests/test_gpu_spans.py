"""Signal spans on the MI355X (include/vbz_gpu.h: vbz_gpu_spans and the two *_signal_spans_batch calls).  edge_first and every word of
edge are held bit for bit to tests/spans_ref.py, result[] and shift_scale beside them, with every table filled with a canary and checked
outside the fitting reads' rows: read lengths around a map byte, a wavefront and a tile, the catalogue of planted runs (test_spans_ref.py
asserts what each holds), the ignored prefix, samples equal to the threshold, uint16 data, clamped key bounds, NaN and infinities, given
constants against both normalisations, ranges (a begin[] straight from the trim call included), every option and frame kind, the
large-read path with runs and gaps across the segment seam, routed and split call shapes, POD5 rows and reads with a row seam inside a
map byte, the cap on edge[], the count-only call, failed reads, and the hand-over into the event call.  Every case asserts a minimum
number of spans in its reference."""
import numpy as np
import pytest
import torch

import events_ref as EV
import norm_ref as R
import oracle_lib as O
import pod5_ref as PD
import pod5_reads_ref as PR
import spans_ref as S
from spans_support import SpanCall, SpanRun, level_table
from test_spans_ref import LEVEL, M
from typed_support import NORMS, Frames, arena, codec, i32, u32
from vbz_compression_amd import _lib, batch

pytestmark = pytest.mark.gpu

TO_END = 0xFFFFFFFF
SEG = 16_384
LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 6145]


def plateaus(rng, T, k=4):
    """noise with up to k planted plateaus of random place and length (one may reach the read's end)"""
    runs = []
    for _ in range(k if T > 40 else 1):
        a = int(rng.integers(0, max(T, 1)))
        runs.append((a, a + int(rng.integers(1, 60))))
    return S.noisy(rng, T, runs)


def levels_of(fr, a=800.0, w=0.0):
    return [(a, w)] * fr.n


# ---- lengths, planted runs, the prefix, equality, uint16, the clamps ---------------------------------------------------------------------------
@pytest.mark.parametrize("P", [(S.ABOVE, 0, 1, 0, 0.0), (S.ABOVE, 9, 3, 0, 2.0), (S.BELOW, 1, 2, 5, -1.5)], ids=["above_d0", "above_d9", "below_d1"])
def test_lengths(P):
    c = codec()
    rng = np.random.default_rng(P[1] + 1)
    reads = [plateaus(rng, T) for T in LENGTHS]
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    lv = [(800.0, 100.0)] * fr.n if P[0] == S.ABOVE else [(400.0, 20.0)] * fr.n   # (below: thr = 370, one sd under the baseline)
    SpanRun(fr, P, lv).check(spans_min=10)
    SpanRun(fr, P, lv, signed=False).check()   # (the same bits taken as uint16)


@pytest.mark.parametrize("D", [0, 1, 9, 65535])
def test_planted_runs(D):
    """the catalogue: runs that begin and end at both edges of a map byte, a wavefront and a tile, at 0 and at T' - 1; gaps of exactly D and
    D + 1 straddling each seam; lengths m - 1 and m before and after a merge"""
    c = codec()
    cat = S.catalogue(D, M)
    fr = Frames(c, [x for _, x in cat], c.options(True, 2, 1, 1))
    SpanRun(fr, (S.ABOVE, D, M, 0, 0.0), [LEVEL] * fr.n).check(spans_min=12)
    SpanRun(fr, (S.BELOW, D, M, 0, 0.0), [(900.0, 0.0)] * fr.n).check(spans_min=12)   # (the baseline is in, the runs are the gaps)


def test_ignore_prefix_inside_a_run_on_its_first_position_and_behind_the_end():
    c = codec()
    reads = [S.baseline(T, [(100, 120), (2040, 2060)]) for T in (130, 2049, 4100)]
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    for p0, least in ((110, 1), (100, 1), (2047, 1), (2048, 1), (5000, 0), (TO_END, 0)):
        r = SpanRun(fr, (S.ABOVE, 0, 1, p0, 0.0), [LEVEL] * fr.n).check(spans_min=least)
        if p0 == 110:
            assert r.want_ed[0].tolist() == [110, 120]
    SpanRun(fr, (S.ABOVE, 0, 1, 13, 0.0), [LEVEL] * fr.n, begin=[95, 3, 2040], end=[TO_END] * 3).check(spans_min=3)   # (p0 counts from the range's first sample)


def test_a_sample_equal_to_the_threshold_is_not_in():
    c = codec()
    x = S.baseline(3000, [(10, 20), (2044, 2052)], base=400, level=402)
    x[30:40] = 401
    fr = Frames(c, [x, x[:9], x[:17]], c.options(True, 2, 1, 1))
    r = SpanRun(fr, (S.ABOVE, 0, 1, 0, 0.0), [(401.0, 0.0)] * 3).check(spans_min=2)
    assert r.want_ed[0].tolist() == [10, 20, 2044, 2052]
    r = SpanRun(fr, (S.BELOW, 0, 1, 0, 0.0), [(401.0, 0.0)] * 3).check(spans_min=3)
    assert r.want_ed[0].tolist() == [0, 10, 20, 30, 40, 2044, 2052, 3000]
    SpanRun(fr, (S.ABOVE, 0, 1, 0, 0.5), [(400.0, 2.0)] * 3).check(spans_min=2)   # (thr = 400 + 0.5 x 2 = 401, through the product)
    SpanRun(fr, (S.ABOVE, 0, 1, 0, 0.0), [(400.5, 0.0)] * 3).check(spans_min=3)   # (a fractional threshold: 401 is in)


def test_uint16_values_above_32768():
    c = codec()
    rng = np.random.default_rng(77)
    reads = [(plateaus(rng, T).astype(np.int32) + 40_000).astype(np.uint16) for T in (9, 2049, 4101, 6151)]
    assert min(int(x.min()) for x in reads) >= 32_768
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    SpanRun(fr, (S.ABOVE, 3, 2, 0, 0.0), levels_of(fr, 40_800.0), signed=False).check(spans_min=4)
    SpanRun(fr, (S.BELOW, 3, 2, 0, 0.0), levels_of(fr, 40_380.0), signed=False).check(spans_min=4)
    SpanRun(fr, (S.ABOVE, 3, 2, 0, 0.0), levels_of(fr, 40_800.0 - 65536.0), signed=True).check(spans_min=4)   # (the same bits as int16)


@pytest.mark.parametrize("signed", [True, False], ids=["int16", "uint16"])
def test_key_bounds_clamped_nan_and_infinities(signed):
    c = codec()
    rng = np.random.default_rng(5)
    reads = [rng.integers(-32768, 32768, T).astype(np.int16) for T in (1, 9, 2049, 4100)]   # (full-range noise: both rails occur)
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    everything = [[3, T] for T in fr.T if T > 3]
    for d, a in ((S.ABOVE, -70_000.0), (S.ABOVE, float("-inf")), (S.BELOW, 70_000.0), (S.BELOW, float("inf")), (S.ABOVE, -1e30), (S.BELOW, 3e38)):
        r = SpanRun(fr, (d, 0, 1, 3, 0.0), levels_of(fr, a), signed=signed).check(spans_min=3)   # key bound 0 / 65 536: one span [p0, T')
        assert [e.tolist() for e in r.want_ed if len(e)] == everything, (d, a)
    for d, a in ((S.ABOVE, 70_000.0), (S.ABOVE, float("inf")), (S.BELOW, -70_000.0), (S.BELOW, float("-inf")), (S.ABOVE, float("nan")),
                 (S.BELOW, float("nan"))):
        r = SpanRun(fr, (d, 0, 1, 0, 0.0), levels_of(fr, a), signed=signed).check(spans_min=0)
        assert int(r.want_first[-1]) == 0
    # the last and the first value that can be in: the rails themselves
    lo, hi = (-32768.0, 32767.0) if signed else (0.0, 65535.0)
    SpanRun(fr, (S.ABOVE, 0, 1, 0, 0.0), levels_of(fr, hi - 0.5), signed=signed).check(spans_min=0)
    SpanRun(fr, (S.BELOW, 0, 1, 0, 0.0), levels_of(fr, lo + 0.5), signed=signed).check(spans_min=0)
    SpanRun(fr, (S.ABOVE, 0, 1, 0, 1.0), [(float("inf"), float("-inf"))] * fr.n, signed=signed).check(spans_min=0)   # (inf - inf: a NaN threshold)


# ---- given constants against a normalisation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stats", [0, 1], ids=["stats_range", "stats_read"])
@pytest.mark.parametrize("norm", ["med_mad", "quantile"])
def test_normalisation_against_given_constants(norm, stats):
    c = codec()
    rng = np.random.default_rng(11)
    reads = [plateaus(rng, T, 6) for T in (0, 1, 9, 513, 2049, 4101, 6151, 20_000)]
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    P = (S.ABOVE, 9, 3, 0, 6.0 if norm == "med_mad" else 2.0)
    bg, en = [3, 0, 8, 11, 0, 2043, 5, 3], [TO_END, TO_END, 9, 500, 2048, TO_END, 6000, 19_000]
    for b, e in ((None, None), (bg, en)):
        if b is None and stats:
            continue
        r = SpanRun(fr, P, norm=NORMS[norm], begin=b, end=e, stats=stats).check(spans_min=6)
        # the statistics call's shift_scale, fed back as level, gives identical tables
        back = SpanRun(fr, P, [(float(a), float(w)) for a, w in r.ss.cpu().numpy()[: fr.n]], begin=b, end=e).check(spans_min=6)
        assert back.tables_bytes() == r.tables_bytes()
        res = torch.full((fr.n,), -8, dtype=torch.int32, device=c.device)
        ss = c.signal_norm(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res, fr.opts, NORMS[norm][1], begin=b, end=e, stats=("read" if stats else "range") if b else None)
        torch.cuda.synchronize()
        assert ss.cpu().numpy().tobytes() == r.ss.cpu().numpy()[: fr.n].tobytes() and u32(res).tolist() == u32(r.result).tolist()
    SpanRun(fr, P, norm=NORMS[norm], with_ss=False).check(spans_min=6)   # (a NULL shift_scale)


# ---- ranges --------------------------------------------------------------------------------------------------------------------------------------
def test_ranges():
    c = codec()
    reads, bg, en = [], [], []
    x = S.baseline(6151, [(0, 5), (96, 130), (2040, 2060), (4090, 4100), (6140, 6151)])
    for b, e in ((8, TO_END), (3, TO_END), (99, 110), (16, 2050), (11, 4095), (2048, 2048), (TO_END, 0), (1, 4), (4099, TO_END), (0, 6145)):
        reads.append(x)
        bg.append(b)
        en.append(e)
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    r = SpanRun(fr, (S.ABOVE, 0, 1, 0, 0.0), [LEVEL] * fr.n, begin=bg, end=en).check(spans_min=15)
    assert r.want_ed[2].tolist() == [0, 11] and r.want_ed[3].tolist()[-2:] == [2024, 2034]   # (begin and end inside a run)
    assert len(r.want_ed[5]) == 0 and len(r.want_ed[6]) == 0                                   # (an empty range of a read that has samples)
    SpanRun(fr, (S.ABOVE, 50, 6, 2, 0.0), [LEVEL] * fr.n, begin=bg, end=None).check(spans_min=8)
    SpanRun(fr, (S.BELOW, 2, 3, 0, 0.0), [LEVEL] * fr.n, begin=None, end=en).check(spans_min=8)


def test_begin_from_the_trim_call_on_the_device():
    c = codec()
    rng = np.random.default_rng(13)
    reads = []
    for T in (3000, 5000, 9000):
        x = S.noisy(rng, T, [(T // 2, T // 2 + 70), (T - 200, T - 150)])
        x[: 400 + T // 20] = (3000 + rng.normal(0, 5, 400 + T // 20)).astype(np.int16)   # (an adapter-like high stretch in front)
        reads.append(x)
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    res = torch.full((fr.n,), -8, dtype=torch.int32, device=c.device)
    begin = c.signal_trim(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res, fr.opts, batch.MED_MAD)
    sp = batch.Spans("above", 5, 10, 0, 0.0)
    level = torch.tensor([[800.0, 0.0]] * fr.n, dtype=torch.float32, device=c.device)
    first, edge = c.signal_spans(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res, fr.opts, sp, level=level, begin=begin)   # (nothing returns to the host in between)
    torch.cuda.synchronize()
    b = u32(begin).tolist()
    assert any(v > 100 for v in b), b
    want_first, want = S.tables(reads, (S.ABOVE, 5, 10, 0, 0.0), [(800.0, 0.0)] * fr.n, b, None)
    assert first.cpu().numpy().tolist() == want_first.tolist() and want_first[-1] >= 12
    assert u32(edge)[: int(want_first[-1])].tolist() == np.concatenate(want).tolist()


# ---- options and frame kinds ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sized", [False, True], ids=["unsized", "sized"])
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("version", [0, 1])
@pytest.mark.parametrize("zz", [True, False], ids=["zz", "nozz"])
def test_options(zz, version, level, sized):
    c = codec()
    rng = np.random.default_rng(version * 8 + level * 4 + sized * 2 + zz)
    reads = [plateaus(rng, T) for T in (0, 1, 9, 65, 2049, 4101, 6151, 20_000)]
    fr = Frames(c, reads, c.options(zz, 2, level, version), sized, slack=6)
    SpanRun(fr, (S.ABOVE, 9, 3, 0, 0.0), levels_of(fr)).check(spans_min=8)
    SpanRun(fr, (S.ABOVE, 9, 3, 0, 6.0), norm=NORMS["med_mad"], begin=[7, 3] * 4, end=[TO_END] * 8).check(spans_min=8)


def test_libzstd_frames():
    c = codec()
    rng = np.random.default_rng(51)
    reads = [plateaus(rng, T) for T in (0, 1, 9, 2049, 4101, 50_000)]
    comp = arena(c, [O.compress(x, O.options(True, 2, 1, 1), sized=True) for x in reads], 64)
    fr = Frames(c, reads, c.options(True, 2, 1, 1), sized=True, comp=comp)
    SpanRun(fr, (S.ABOVE, 9, 3, 0, 0.0), levels_of(fr)).check(spans_min=6)
    SpanRun(fr, (S.BELOW, 0, 2, 4, -1.0), norm=NORMS["quantile"], begin=[8] * fr.n, end=[TO_END] * fr.n).check(spans_min=6)


# ---- the other decode paths -----------------------------------------------------------------------------------------------------------------
def large_reads(D):
    """reads around the segment's 16 384 samples: a run across the seam, and pairs whose gaps of D and D + 1 straddle it"""
    reads = []
    for T in (SEG - 1, SEG, SEG + 1, 40_000):
        runs = [(100, 140), (T - 30, T)]
        if T > SEG + 200:
            runs += [(SEG - 20, SEG + 20), (2 * SEG - 3, 2 * SEG)]
        reads.append(S.baseline(T, runs))
    for gap in (D, D + 1):
        reads.append(S.pair(40_000, SEG, gap, M))
        reads.append(S.pair(40_000, 2 * SEG, gap, M - 1))
    return reads


@pytest.mark.parametrize("segmented", [1, 0])
def test_large_reads_on_forced_paths(segmented):
    c = codec(VBZ_HIP_SEGMENTED=segmented)
    for D in (0, 9):
        reads = large_reads(D)
        fr = Frames(c, reads, c.options(True, 2, 1, 1))
        r = SpanRun(fr, (S.ABOVE, D, M, 0, 0.0), [LEVEL] * fr.n).check(spans_min=12)
        assert [SEG - 20, SEG + 20] in r.want_ed[3].reshape(-1, 2).tolist()
        assert len(r.want_ed[4]) == 2 and len(r.want_ed[6]) == 4 and len(r.want_ed[5]) == 2 and len(r.want_ed[7]) == 0
        SpanRun(fr, (S.ABOVE, D, M, 3, 0.0), [LEVEL] * fr.n, begin=[5, 1, 4097, 3] * 2, end=[TO_END, TO_END, SEG, 2 * SEG - 1] * 2).check(spans_min=6)
    rng = np.random.default_rng(3)
    fr = Frames(c, [plateaus(rng, T, 8) for T in (SEG + 1, 40_000, 3 * SEG)], c.options(True, 2, 1, 1))
    for name in ("med_mad", "quantile"):   # (behind the counting passes: the large-read path's slab, or LDS)
        SpanRun(fr, (S.ABOVE, 9, 3, 0, 6.0 if name == "med_mad" else 2.0), norm=NORMS[name]).check(spans_min=6)
    fr = Frames(c, [plateaus(rng, T, 8) for T in (SEG + 1, 40_000)], c.options(False, 2, 0, 0))
    SpanRun(fr, (S.ABOVE, 9, 3, 0, 0.0), levels_of(fr)).check(spans_min=4)   # (no zig-zag, level 0: the other instantiation)


def mixed_batch(n, at, seed):
    rng = np.random.default_rng(seed)
    reads = [plateaus(rng, int(rng.integers(500, 5000))) for _ in range(n)]
    reads[at] = plateaus(rng, 262_144, 40)
    reads[at][SEG - 5 : SEG + 5] = 1300
    return reads


def test_routed_long_read_among_small_ones():
    c = codec()
    reads = mixed_batch(41, 17, 41)
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    r = SpanRun(fr, (S.ABOVE, 9, 3, 0, 0.0), levels_of(fr)).check(spans_min=60)
    assert len(r.want_ed[17]) >= 40
    bg, en = [8 if i % 2 else 3 for i in range(fr.n)], [TO_END if i % 3 else 2000 for i in range(fr.n)]
    bg[17], en[17] = 2003, 260_000
    SpanRun(fr, (S.ABOVE, 9, 3, 0, 6.0), norm=NORMS["med_mad"], begin=bg, end=en).check(spans_min=60)


def test_split_batch():
    """the upper half finds its own maps and levels"""
    rng = np.random.default_rng(31)
    reads = [plateaus(rng, int(rng.integers(50, 3000))) for _ in range(128)]
    lv = [(700.0 + i, 1.0) for i in range(128)]
    outs = []
    for c in (codec(VBZ_HIP_SPLIT_MIN=64), codec(VBZ_HIP_SPLIT_MIN=0)):
        fr = Frames(c, reads, c.options(True, 2, 1, 1))
        r = SpanRun(fr, (S.ABOVE, 9, 3, 0, 2.0), lv).check(spans_min=100)
        n = SpanRun(fr, (S.ABOVE, 9, 3, 0, 6.0), norm=NORMS["med_mad"]).check(spans_min=100)
        outs.append(r.tables_bytes() + n.tables_bytes())
    assert outs[0] == outs[1]


@pytest.mark.parametrize("at", [30, 150], ids=["lower-half", "upper-half"])
def test_routed_long_read_in_a_split_batch(at):
    """both cuts of one call: the routed read finds its map, its level and its range through the routing map, the upper half through its
    offset tables"""
    reads = mixed_batch(200, at, 43)
    lv = [(700.0 + i, 1.0) for i in range(200)]
    bg, en = [9 if i % 2 else 3 for i in range(200)], [TO_END if i % 3 else 2000 for i in range(200)]
    bg[at], en[at] = 2003, 260_000
    outs = []
    for c in (codec(VBZ_HIP_SPLIT_MIN=64), codec(VBZ_HIP_SPLIT_MIN=0, VBZ_HIP_ROUTING=0)):
        fr = Frames(c, reads, c.options(True, 2, 1, 1))
        r = SpanRun(fr, (S.ABOVE, 9, 3, 0, 2.0), lv, begin=bg, end=en).check(spans_min=200)
        assert len(r.want_ed[at]) >= 40
        n = SpanRun(fr, (S.ABOVE, 9, 3, 0, 6.0), norm=NORMS["med_mad"], begin=bg, end=en, stats=1).check(spans_min=200)
        outs.append(r.tables_bytes() + n.tables_bytes())
    assert outs[0] == outs[1]


# ---- POD5 ---------------------------------------------------------------------------------------------------------------------------------------
def test_pod5_rows_as_reads():
    c = codec()
    rng = np.random.default_rng(61)
    rows = [plateaus(rng, T) for T in (0, 1, 7, 9, 2047, 2049, 4101, 6151)]
    fr = Frames(c, rows, batch.pod5_options(), comp=arena(c, [PD.compress_row(x) for x in rows], 64))
    SpanRun(fr, (S.ABOVE, 9, 3, 0, 0.0), levels_of(fr)).check(spans_min=6)
    SpanRun(fr, (S.ABOVE, 9, 3, 0, 6.0), norm=NORMS["med_mad"], begin=[3] * fr.n, end=[6000] * fr.n).check(spans_min=6)
    SpanRun(fr, (S.BELOW, 0, 1, 2, 0.0), levels_of(fr, 33_150.0), signed=False).check(spans_min=6)


POD5_SHAPES = [[3000], [2049, 1], [1, 7, 9, 2047, 2049], [2047, 9, 7, 1, 2049], [], [0, 0], [9, 0, 2047], [13, 14, 30]]
POD5_D = 4


def pod5_rows(shapes):
    """reads whose rows' sample counts are no multiples of 8: at every other row seam a run across it, at the others a pair whose gap of
    POD5_D straddles it -- the seams at 13 and 27 of the last read, and at 17 of the third, lie inside one map byte"""
    rows, first = [], []
    for lens in shapes:
        first.append(len(rows))
        T = sum(lens)
        cum = np.cumsum([0] + lens)
        runs = [(T - 4, T)]
        for k, q in enumerate(cum[1:-1]):
            if 8 <= q <= T - 8:
                runs += [(q - 3, q + 3)] if k % 2 == 0 else [(q - 5, q - 2), (q - 2 + POD5_D, q + 1 + POD5_D)]
        x = S.baseline(T, runs)
        rows += [x[cum[k] : cum[k + 1]].copy() for k in range(len(lens))]
    return rows, first


@pytest.mark.parametrize("segmented", [0, 1])
def test_pod5_reads(segmented):
    c = codec(VBZ_HIP_SEGMENTED=segmented)
    rows, first = pod5_rows(POD5_SHAPES)
    frames = [PD.compress_row(x) for x in rows]
    n = len(first)
    for D in (POD5_D, POD5_D - 1):
        call = SpanCall(c, frames, rows, first, (S.ABOVE, D, 3, 0, 0.0), [LEVEL] * n)
        assert call.call() == 0, c.L.vbz_gpu_last_error(c.ctx)
        call.check(spans_min=10)
    assert [10, 16] in call.want_ed[7].reshape(-1, 2).tolist()   # (the run across the seam at 13, inside the map byte of positions 8 ... 15)
    rng = np.random.default_rng(7)
    noise = [S.noisy(rng, len(x), [(len(x) // 2, len(x) // 2 + 9)]) for x in rows]
    nframes = [PD.compress_row(x) for x in noise]
    for name, stats in (("med_mad", 0), ("quantile", 1)):
        bg, en = [5, 3, 1, 2040, 0, 0, 3, 2], [TO_END, 2049, 4000, TO_END, 0, 7, 2000, 40]
        call = SpanCall(c, nframes, noise, first, (S.ABOVE, 2, 2, 1, 3.0), norm=NORMS[name], begin=bg, end=en, stats=stats)
        assert call.call() == 0, c.L.vbz_gpu_last_error(c.ctx)
        call.check(spans_min=4)
    call = SpanCall(c, frames, rows, first, (S.BELOW, 0, 2, 3, 0.0), [LEVEL] * n, signed=False, begin=[5, 3, 1, 2040, 0, 0, 3, 2], end=None)
    assert call.call() == 0, c.L.vbz_gpu_last_error(c.ctx)
    call.check(spans_min=10)


def test_pod5_read_with_a_failing_row_counts_none():
    c = codec()
    rows, first = pod5_rows([[3000], [1001, 903, 805], [2049, 100]])
    frames = [PD.compress_row(x) for x in rows]
    frames[2] = frames[2][: len(frames[2]) // 2]   # the middle row of read 1 cut off
    for cap, norm in ((None, None), (3, None), (None, NORMS["med_mad"])):
        kw = dict(levels=[LEVEL] * 3) if norm is None else dict(norm=norm)
        rws = rows if norm is None else [S.noisy(np.random.default_rng(i), len(x), [(len(x) // 2, len(x) // 2 + 9)]) for i, x in enumerate(rows)]
        frs = frames if norm is None else [PD.compress_row(x) for x in rws[:2]] + [frames[2]] + [PD.compress_row(x) for x in rws[3:]]
        call = SpanCall(c, frs, rws, first, (S.ABOVE, 0, 2, 0, 0.0 if norm is None else 6.0), failed={1}, cap=cap, **kw)
        assert call.call() == 0, c.L.vbz_gpu_last_error(c.ctx)
        call.check(row_expect={2: 0xFFFFFFFF}, spans_min=2)
        assert call.want_first[2] == call.want_first[1]
        assert call.refused == (set() if cap is None else {2})


@pytest.mark.parametrize("segmented", [0, 1])
def test_pod5_rows_that_begin_inside_a_map_byte(segmented):
    """One read of rows of 13, 2 049 and 5 samples -- a partial map byte, a tile seam, a tail: its second and third rows begin at 13 and
    2 062, inside a byte of the map -- and beside it the same read with its middle row cut off, which owns nothing.  With given constants
    (the pass writes the verdicts) and behind a normalisation (it owes none), over the whole read and over a range that begins and ends
    inside a row.  (test_pod5_reads has such seams with given constants, and behind a normalisation only with a range; its failing read's
    rows run on the default path alone.)"""
    c = codec(VBZ_HIP_SEGMENTED=segmented)
    rows, first = pod5_rows([[13, 2049, 5], [13, 2049, 5]])
    rng = np.random.default_rng(97)
    noise = [S.noisy(rng, len(x), [(len(x) // 2, len(x) // 2 + 9)]) for x in rows]
    for rws, kw, P in ((rows, dict(levels=[LEVEL] * 2), (S.ABOVE, 0, 1, 0, 0.0)), (noise, dict(norm=NORMS["med_mad"]), (S.ABOVE, 0, 2, 0, 6.0))):
        frames = [PD.compress_row(x) for x in rws]
        frames[4] = frames[4][: len(frames[4]) // 2]   # the middle row of read 1 cut off
        for bg, en in ((None, None), ([11, 11], [2064, 2064])):
            call = SpanCall(c, frames, rws, first, P, failed={1}, begin=bg, end=en, **kw)
            assert call.call() == 0, c.L.vbz_gpu_last_error(c.ctx)
            call.check(row_expect={4: 0xFFFFFFFF}, spans_min=2)
            assert call.want_first[2] == call.want_first[1] and call.refused == set()
            if rws is rows and bg is None:
                assert call.want_ed[0].tolist() == [10, 16, 2063, 2067]   # (the run across the seam at 13, inside the map byte of 8 ... 15)


# ---- the cap on edge[], the count-only call, failed reads -------------------------------------------------------------------------------------
def cap_case(c):
    rng = np.random.default_rng(19)
    return Frames(c, [plateaus(rng, T, 5) for T in (3000, 0, 700, 5000, 640)], c.options(True, 2, 1, 1))


CAP_P = (S.ABOVE, 2, 2, 0, 0.0)


def test_edge_cap_exact_and_one_pair_short():
    c = codec()
    fr = cap_case(c)
    total = int(SpanRun(fr, CAP_P, levels_of(fr)).check(spans_min=5).want_first[-1])
    r = SpanRun(fr, CAP_P, levels_of(fr), cap=total - 2).check()
    assert r.refused == {4}   # exactly the reads whose pairs end beyond the cap; its words of edge keep the canary (Tables.check)
    r = SpanRun(fr, CAP_P, levels_of(fr), cap=total - 1).check()
    assert r.refused == {4}
    r = SpanRun(fr, CAP_P, levels_of(fr), cap=int(r.want_first[3])).check()
    assert r.refused == {3, 4}
    r = SpanRun(fr, CAP_P, levels_of(fr), cap=int(r.want_first[1]) - 1).check()
    assert r.refused == {0, 2, 3, 4}   # (read 1 has no sample and no span: nothing to refuse)
    SpanRun(fr, CAP_P, levels_of(fr), cap=total + 9).check()
    SpanRun(fr, (S.ABOVE, 2, 2, 0, 6.0), norm=NORMS["med_mad"], cap=3).check()


def test_count_only_call():
    c = codec()
    fr = cap_case(c)
    r = SpanRun(fr, CAP_P, levels_of(fr), count_only=True).check(spans_min=5)
    assert r.refused == set() and u32(r.result)[: fr.n].tolist() == [2 * T for T in fr.T]
    SpanRun(fr, (S.ABOVE, 2, 2, 0, 6.0), norm=NORMS["med_mad"], count_only=True).check(spans_min=5)


def test_failed_reads_have_no_rows():
    c = codec()
    fr = cap_case(c)
    size = fr.size.clone()
    size[2] = int(u32(fr.size)[2]) // 2   # the frame of read 2 cut off in its middle
    dst = torch.zeros(fr.dst_bytes + 64, dtype=torch.uint8, device=c.device)
    res16 = torch.full((fr.n,), -8, dtype=torch.int32, device=c.device)
    c.decompress(fr.src, fr.off, size, dst, fr.doff, fr.dcap, res16, fr.opts)
    torch.cuda.synchronize()
    un = u32(res16).tolist()
    assert _lib.is_error(un[2])
    fr.size = size
    r = SpanRun(fr, CAP_P, levels_of(fr), failed={2}).check(expect={2: un[2]}, spans_min=4)
    assert r.want_first[3] == r.want_first[2]
    SpanRun(fr, CAP_P, levels_of(fr), failed={2}, count_only=True).check(expect={2: un[2]}, spans_min=4)
    SpanRun(fr, (S.ABOVE, 2, 2, 0, 6.0), norm=NORMS["med_mad"], failed={2}).check(expect={2: un[2]}, spans_min=4)


# ---- the hand-over and the Python methods ------------------------------------------------------------------------------------------------------
def test_hand_over_into_the_event_call():
    """edge_first and edge go from the span call straight into signal_events on the device, with the same ranges: even rows are the spans'
    records, odd rows the stretches between them, the last one running to T'"""
    c = codec()
    rng = np.random.default_rng(83)
    reads = [S.noisy(rng, T, [(T // 4, T // 4 + 50), (T // 2, T // 2 + 7), (T - 90, T - 40)]) for T in (0, 200, 2049, 4101, 20_000)]
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    sp = batch.Spans("above", 5, 3, 0, 0.0)
    level = torch.tensor([[800.0, 0.0]] * fr.n, dtype=torch.float32, device=c.device)
    for bg, en in ((None, None), ([3, 1, 7, 2047, 5], [TO_END, 190, 2000, TO_END, 19_990])):
        res = torch.full((fr.n,), -8, dtype=torch.int32, device=c.device)
        first, edge = c.signal_spans(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res, fr.opts, sp, level=level, begin=bg, end=en)
        mean, sd, n, mom = c.signal_events(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res, fr.opts, first, edge, begin=bg, end=en, moments=True)
        torch.cuda.synchronize()
        want_first, ed = S.tables(reads, (S.ABOVE, 5, 3, 0, 0.0), [(800.0, 0.0)] * fr.n, bg, en)
        total = int(want_first[-1])
        assert total >= 12 and first.cpu().numpy().tolist() == want_first.tolist() and u32(edge)[:total].tolist() == np.concatenate(ed).tolist()
        want = [EV.event_rows(x, None if bg is None else bg[i], None if en is None else en[i], ed[i].tolist(), 0.0, 1.0) for i, x in enumerate(reads)]
        rows, moms = np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want])
        assert (mean.cpu().numpy().view(np.uint32)[:total] == rows[:, 0]).all() and (sd.cpu().numpy().view(np.uint32)[:total] == rows[:, 1]).all()
        assert (n.cpu().numpy().view(np.uint32)[:total] == rows[:, 2]).all() and (mom.cpu().numpy()[:total] == moms).all()
        dwell = n.cpu().numpy().view(np.uint32)[:total]
        k = int(want_first[2])
        assert dwell[k] == ed[2][1] - ed[2][0] and dwell[k + 1] == ed[2][2] - ed[2][1]   # (a span's dwell, then the gap behind it)
        assert u32(res).tolist() == [2 * T for T in fr.T]


def test_python_methods():
    c = codec()
    dev = c.device
    rng = np.random.default_rng(2)
    reads = [plateaus(rng, T, 6) for T in (0, 1, 65, 2049, 6151)]
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    res = torch.full((fr.n,), -8, dtype=torch.int32, device=dev)
    sp = batch.Spans("above", 9, 3, 0, 6.0)
    first, edge, ss = c.signal_spans(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res, fr.opts, sp, norm=batch.MED_MAD, shift_scale=True)
    torch.cuda.synchronize()
    lv = [R.shift_scale(x, R.BONITO) for x in reads]
    want_first, ed = S.tables(reads, (S.ABOVE, 9, 3, 0, 6.0), lv)
    assert first.dtype == torch.int64 and edge.dtype == torch.int32 and first.device == dev and edge.device == dev
    assert int(edge.numel()) == sum(sp.max_edges(T) for T in fr.T) >= int(want_first[-1]) >= 8   # (the bound sizes edge)
    assert first.cpu().numpy().tolist() == want_first.tolist() and u32(edge)[: int(want_first[-1])].tolist() == np.concatenate(ed).tolist()
    assert u32(res).tolist() == [2 * T for T in fr.T]
    assert ss.cpu().numpy().tobytes() == np.array(lv, np.float32).tobytes()
    first1, edge1 = c.signal_spans(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res, fr.opts, sp, level=ss)   # (shift_scale as level)
    first0, none = c.signal_spans(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res, fr.opts, sp, level=ss, edge_cap=0)   # the count-only call
    torch.cuda.synchronize()
    assert torch.equal(first1, first) and torch.equal(edge1[: int(want_first[-1])], edge[: int(want_first[-1])])
    assert none is None and first0.cpu().numpy().tolist() == want_first.tolist()
    # POD5
    prow, pfirst = pod5_rows([[13, 7, 1, 2047, 2049], [800, 0, 800], [300] * 10, []])
    src, off, size = arena(c, [PD.compress_row(x) for x in prow], 16)
    res = torch.full((len(prow),), -8, dtype=torch.int32, device=dev)
    rr = torch.full((len(pfirst),), -8, dtype=torch.int32, device=dev)
    level = level_table(c, [LEVEL] * len(pfirst), len(pfirst))[: len(pfirst)].contiguous()
    first, edge, rr2 = c.pod5_signal_spans(src, off, size, i32([len(x) for x in prow]).to(dev), pfirst, res, batch.Spans("above", 2, 3), signed=False,
                                           level=level, read_result=rr)
    torch.cuda.synchronize()
    sig = [x.view(np.uint16) for x in PR.read_signals(prow, pfirst)]
    want_first, ed = S.tables(sig, (S.ABOVE, 2, 3, 0, 0.0), [LEVEL] * len(sig))
    assert first.cpu().numpy().tolist() == want_first.tolist() and u32(edge)[: int(want_first[-1])].tolist() == np.concatenate(ed).tolist()
    assert want_first[-1] >= 10 and u32(rr2).tolist() == [2 * len(x) for x in sig] and u32(res).tolist() == [2 * len(x) for x in prow]
