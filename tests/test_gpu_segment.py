"""Signal segmentation on the MI355X (include/vbz_gpu.h: vbz_gpu_segmentation and the two *_signal_segment_batch calls).  event_first and
every start are held bit for bit to tests/segment_ref.py, result[] beside them, with both tables filled with a canary and checked
outside the fitting reads' rows: read lengths around a tile (2 048), the halo H = max(w1, w2) + r and the paired-tile loop, planted
noise-free steps at the first and last positions a detector sees, at the tile seams and at the edges of a map byte, square waves whose
equal scores tie across a tile seam, every parameter corner, uint16 data, every option and frame kind, the large-read path, routed and
split call shapes, ranges (a begin[] straight from the trim call included), POD5 rows and reads, the cap on start[], the count-only
call, failed reads, and the hand-over into the event call.  Every case asserts that its reference lists more than one row for some read."""
import numpy as np
import pytest
import torch

import events_ref as EV
import oracle_lib as O
import pod5_ref as PD
import pod5_reads_ref as PR
import segment_ref as S
from segment_support import SegCall, SegRun
from typed_support import Frames, arena, codec, i32, u32
from vbz_compression_amd import _lib, batch

pytestmark = pytest.mark.gpu

TO_END = 0xFFFFFFFF
PARAMS = [(3, 6, 4.0, 9.0, 2), (1, 0, 1.5, 1.0, 1), (32, 32, 2.0, 3.0, 32), (3, 6, 4.0, 9.0, 32)]
SEG = 16_384


def halo(P):
    return max(P[0], P[1]) + P[4]


def steps(rng, T, lo=3, hi=30, noise=6.0):
    """a step signal of random dwell lo ... hi under Gaussian noise"""
    x, p = np.zeros(T), 0
    while p < T:
        d = int(rng.integers(lo, hi + 1))
        x[p : p + d] = rng.uniform(-600, 900)
        p += d
    return np.clip(x + rng.normal(0, noise, T), -32768, 32767).astype(np.int16)


def planted(T, at, lo=-250, hi=640):
    """noise-free plateaus with a step at every position of `at`"""
    x = np.full(T, lo, np.int16)
    for k, q in enumerate(sorted(at)):
        x[q:] = hi if k % 2 == 0 else lo
    return x


def square(T, half, lo=100, hi=500):
    return np.where((np.arange(T) // half) % 2 == 0, lo, hi).astype(np.int16)


def lengths(P):
    H = halo(P)
    return [0, 1, 5, 11, 12, 2047, 2048, 2049, 2048 - H, 2048 + H, 4095, 4096, 4097, 6143, 6144, 6145]


# ---- lengths, planted steps, ties, parameters, uint16 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", PARAMS, ids=lambda P: "w%d_%d_r%d" % (P[0], P[1], P[4]))
def test_lengths(P):
    c = codec()
    rng = np.random.default_rng(P[0] + P[4])
    reads = [steps(rng, T, 3, 40 if P[0] < 32 else 200) for T in lengths(P)]
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    SegRun(fr, P).check()
    SegRun(fr, P, signed=False).check()   # (the same bits as uint16: another signal, values >= 32 768 among them)


@pytest.mark.parametrize("P", PARAMS, ids=lambda P: "w%d_%d_r%d" % (P[0], P[1], P[4]))
def test_planted_steps(P):
    """a noise-free step at the first and the last position a detector sees, at the tile seams, at 4 096 and at both edges of a map byte:
    each is a boundary, exactly there"""
    c = codec()
    w1, T = P[0], 6000
    spots = [2047, 2048, 2049, 4096, 1007, 1008]   # (1 007 = 7 mod 8, 1 008 = 0 mod 8)
    reads = [planted(T, [w1, q, T - w1]) for q in spots]
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    r = SegRun(fr, P).check(rows_min=4)
    for st, q in zip(r.want_st, spots):
        assert {w1, q, T - w1} <= set(st.tolist()), (P, q, st.tolist())


@pytest.mark.parametrize("r", [2, 4])
def test_square_waves_tie_across_a_tile_seam(r):
    """equal scores >= 1 within r of each other (tests/test_segment_ref.py asserts they occur), at every phase against the seam at 2 048"""
    c = codec()
    P = (3, 6, 2.0, 4.0, r)
    reads = [square(4200, half)[ph:] for half in (3, 4, 5) for ph in range(0, 2 * half)]
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    SegRun(fr, P).check(rows_min=100)
    s = S.scores(reads[2 * 3], P)   # (half-period 4)
    assert any(s[q] >= 1 and s[q] == s[j] for q in range(2040, 2056) for j in range(q + 1, q + r + 1))


def test_uint16_values_above_32768():
    c = codec()
    rng = np.random.default_rng(77)
    reads = [(steps(rng, T).astype(np.int32) + 40_000).astype(np.uint16) for T in (9, 2049, 4101, 6151)]
    assert min(int(x.min()) for x in reads) >= 32_768
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    SegRun(fr, signed=False).check()
    SegRun(fr, signed=True).check()   # (the same bits as int16: the values wrap, another signal)


# ---- options and frame kinds ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sized", [False, True], ids=["unsized", "sized"])
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("version", [0, 1])
@pytest.mark.parametrize("zz", [True, False], ids=["zz", "nozz"])
def test_options(zz, version, level, sized):
    c = codec()
    rng = np.random.default_rng(version * 8 + level * 4 + sized * 2 + zz)
    reads = [steps(rng, T) for T in (0, 1, 9, 65, 2049, 4101, 6151, 20_000)]
    fr = Frames(c, reads, c.options(zz, 2, level, version), sized, slack=6)
    SegRun(fr).check()
    SegRun(fr, PARAMS[2], [7, 3] * 4, [TO_END] * 8, signed=False).check()


def test_libzstd_frames():
    c = codec()
    rng = np.random.default_rng(51)
    reads = [steps(rng, T) for T in (0, 1, 9, 2049, 4101, 50_000)]
    comp = arena(c, [O.compress(x, O.options(True, 2, 1, 1), sized=True) for x in reads], 64)
    fr = Frames(c, reads, c.options(True, 2, 1, 1), sized=True, comp=comp)
    SegRun(fr).check()
    SegRun(fr, PARAMS[3], [8] * fr.n, [TO_END] * fr.n).check()


# ---- the other decode paths -----------------------------------------------------------------------------------------------------------------
def large_reads(P):
    H = halo(P)
    rng = np.random.default_rng(23)
    reads = []
    for T in (SEG - H, SEG + H, 2 * SEG, 3 * SEG + 5):
        x = steps(rng, T, 20, 60, 3.0)
        for k in range(1, T // SEG + 1):   # noise-free steps at k SEG - 1, k SEG and k SEG + 1, one seam each
            q = k * SEG + (k % 3) - 1
            if q < T:
                x[q - 40 : q], x[q : q + 40] = -300, 800   # (the last one has the read's last 6 samples behind it)
        reads.append(x)
    return reads


@pytest.mark.parametrize("segmented", [1, 0])
def test_large_reads_on_forced_paths(segmented):
    c = codec(VBZ_HIP_SEGMENTED=segmented)
    for P in (PARAMS[0], PARAMS[2]):
        reads = large_reads(P)
        fr = Frames(c, reads, c.options(True, 2, 1, 1))
        r = SegRun(fr, P).check()
        assert SEG in r.want_st[2].tolist() and 2 * SEG + 1 in r.want_st[3].tolist()
        SegRun(fr, P, [5, 1, 4097, 3], [TO_END, TO_END, 2 * SEG - 1, 3 * SEG]).check()   # (odd begins: the groups straddle the segments)


def test_routed_long_read_among_small_ones():
    c = codec()
    rng = np.random.default_rng(41)
    reads = [steps(rng, int(rng.integers(500, 5000))) for _ in range(41)]
    reads[17] = steps(rng, 262_144)
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    r = SegRun(fr).check()
    assert len(r.want_st[17]) > 5000
    bg, en = [8 if i % 2 else 3 for i in range(fr.n)], [TO_END if i % 3 else 2000 for i in range(fr.n)]
    bg[17], en[17] = 2003, 260_000
    SegRun(fr, PARAMS[3], bg, en).check()


def test_split_batch():
    """the upper half finds its own maps and row counts"""
    rng = np.random.default_rng(31)
    reads = [steps(rng, int(rng.integers(50, 3000))) for _ in range(128)]
    outs = []
    for c in (codec(VBZ_HIP_SPLIT_MIN=64), codec(VBZ_HIP_SPLIT_MIN=0)):
        fr = Frames(c, reads, c.options(True, 2, 1, 1))
        r = SegRun(fr).check()
        outs.append((r.t.first.cpu().numpy().tobytes(), r.t.start.cpu().numpy().tobytes()))
    assert outs[0] == outs[1]


@pytest.mark.parametrize("ranged", [False, True], ids=["whole", "ranged"])
@pytest.mark.parametrize("at", [30, 150], ids=["lower-half", "upper-half"])
def test_routed_long_read_in_a_split_batch(at, ranged, monkeypatch):
    """both cuts of one call: the routed read finds its map, its row count and its range through the routing map, the upper half through
    its offset tables"""
    rng = np.random.default_rng(43)
    reads = [steps(rng, int(rng.integers(500, 5000))) for _ in range(200)]
    reads[at] = steps(rng, 262_144)
    bg = en = None
    if ranged:   # (odd begins)
        bg, en = [9 if i % 2 else 3 for i in range(200)], [TO_END if i % 3 else 2000 for i in range(200)]
        bg[at], en[at] = 2003, 260_000
    outs = []
    # (shape: the call's launches of route and svb_decode -- routed and two halves, the routed group's own not counted; one group.  The
    # context made here has seen no frames, so its first call runs as halves whatever an earlier call held: a context that saw mostly
    # frames left to the one-wavefront decoder runs its next call as one group)
    monkeypatch.setenv("VBZ_HIP_SPLIT_MIN", "64")
    unused = batch.GpuCodec(0)
    monkeypatch.delenv("VBZ_HIP_SPLIT_MIN")
    for c, shape in ((unused, (1, 2)), (codec(VBZ_HIP_SPLIT_MIN=64), None), (codec(VBZ_HIP_SPLIT_MIN=0, VBZ_HIP_ROUTING=0), (0, 1))):
        fr = Frames(c, reads, c.options(True, 2, 1, 1))
        c.profile_reset()
        c.profile(True)
        r = SegRun(fr, PARAMS[3] if ranged else S.DEFAULT, bg, en)
        c.profile(False)
        prof = {k: v[0] for k, v in c.profile_read().items()}
        assert shape is None or (prof.get("route", 0), prof["svb_decode"]) == shape, sorted(prof.items())
        r.check()
        assert len(r.want_st[at]) > 3000
        outs.append((r.t.first.cpu().numpy().tobytes(), r.t.start.cpu().numpy().tobytes(), u32(r.result).tolist()))
    assert outs[0] == outs[2] and outs[1] == outs[2]


# ---- ranges -------------------------------------------------------------------------------------------------------------------------------------
def test_ranges():
    c = codec()
    rng = np.random.default_rng(29)
    reads, bg, en = [], [], []
    for T in (9, 65, 2049, 4101, 6151):
        x = steps(rng, T, 3, 20)
        for b, e in ((3, TO_END), (0, max(T - 3, 0)), (5, max(T - 100, 0)), (2047, TO_END), (2048, 2048), (TO_END, 0), (1, 30)):
            reads.append(x)
            bg.append(b)
            en.append(e)
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    r = SegRun(fr, S.DEFAULT, bg, en).check()
    assert any(len(v) == 0 for v, T in zip(r.want_st, fr.T) if T)   # (an empty range of a read that has samples: no row)
    SegRun(fr, PARAMS[2], bg, None).check()
    SegRun(fr, PARAMS[1], None, en).check()


def test_begin_from_the_trim_call_on_the_device():
    c = codec()
    rng = np.random.default_rng(13)
    reads = []
    for T in (3000, 5000, 9000):
        x = steps(rng, T, 5, 25)
        x[: 400 + T // 20] = (3000 + rng.normal(0, 5, 400 + T // 20)).astype(np.int16)   # (an adapter-like high stretch in front)
        reads.append(x)
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    res = torch.full((fr.n,), -8, dtype=torch.int32, device=c.device)
    begin = c.signal_trim(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res, fr.opts, batch.MED_MAD)
    first, start = c.signal_segment(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res, fr.opts, begin=begin)   # (nothing returns to the host in between)
    torch.cuda.synchronize()
    b = u32(begin).tolist()
    assert any(v > 100 for v in b), b
    want_first, want = S.tables(reads, b, None)
    assert first.cpu().numpy().tolist() == want_first.tolist() and want_first[-1] > 100
    assert u32(start)[: int(want_first[-1])].tolist() == np.concatenate(want).tolist()


# ---- POD5 ---------------------------------------------------------------------------------------------------------------------------------------
def test_pod5_rows_as_reads():
    c = codec()
    rng = np.random.default_rng(61)
    rows = [steps(rng, T) for T in (0, 1, 7, 9, 2047, 2049, 4101, 6151)]
    fr = Frames(c, rows, batch.pod5_options(), comp=arena(c, [PD.compress_row(x) for x in rows], 64))
    SegRun(fr).check()
    SegRun(fr, PARAMS[2], [3] * fr.n, [6000] * fr.n, signed=False).check()


POD5_SHAPES = [[3000], [2049, 1], [1, 7, 9, 2047, 2049], [2047, 9, 7, 1, 2049], [], [0, 0], [9, 0, 2047]]


def pod5_rows(seed, shapes):
    """reads whose rows' seams carry noise-free steps (every other seam) over a step signal"""
    rng = np.random.default_rng(seed)
    rows, first = [], []
    for lens in shapes:
        first.append(len(rows))
        x = steps(rng, sum(lens), 4, 25)
        cum = np.cumsum([0] + lens)
        for k, q in enumerate(cum[1:-1]):
            if k % 2 == 0 and 12 <= q <= len(x) - 12:
                x[q - 12 : q], x[q : q + 12] = -400, 700
        rows += [x[cum[k] : cum[k + 1]].copy() for k in range(len(lens))]
    return rows, first


@pytest.mark.parametrize("segmented", [0, 1])
def test_pod5_reads(segmented):
    c = codec(VBZ_HIP_SEGMENTED=segmented)
    rows, first = pod5_rows(71, POD5_SHAPES)
    frames = [PD.compress_row(x) for x in rows]
    call = SegCall(c, frames, rows, first)
    assert call.call() == 0, c.L.vbz_gpu_last_error(c.ctx)
    call.check()
    assert 17 in call.want_st[2].tolist()   # (the planted step on the seam between the rows of 9 and of 2 047 samples)
    for P, signed in ((PARAMS[1], True), (PARAMS[2], False), (PARAMS[3], True)):
        call = SegCall(c, frames, rows, first, P, signed=signed)
        assert call.call() == 0, c.L.vbz_gpu_last_error(c.ctx)
        call.check()
    bg, en = [5, 3, 1, 2040, 0, 0, 3], [TO_END, 2049, 4000, TO_END, 0, 7, 9]
    call = SegCall(c, frames, rows, first, S.DEFAULT, bg, en)
    assert call.call() == 0, c.L.vbz_gpu_last_error(c.ctx)
    call.check()


def test_pod5_read_with_a_failing_row_counts_none():
    c = codec()
    rows, first = pod5_rows(72, [[3000], [1000, 900, 800], [2049, 100]])
    frames = [PD.compress_row(x) for x in rows]
    frames[2] = frames[2][: len(frames[2]) // 2]   # the middle row of read 1 cut off
    for cap in (None, 5):
        call = SegCall(c, frames, rows, first, failed={1}, cap=cap)
        assert call.call() == 0, c.L.vbz_gpu_last_error(c.ctx)
        call.check(row_expect={2: 0xFFFFFFFF})
        assert call.want_first[2] == call.want_first[1]
        assert call.refused == (set() if cap is None else {0, 2})


@pytest.mark.parametrize("segmented", [0, 1])
def test_pod5_rows_that_begin_inside_a_map_byte(segmented):
    """One read of rows of 13, 2 049 and 5 samples -- a partial map byte, a tile seam, a tail: its second and third rows begin at 13 and
    2 062 -- and beside it the same read with its middle row cut off, which gets no row; over the whole read and over a range that begins
    and ends inside a row.  (test_pod5_reads has such seams; its failing read's rows run on the default path alone and begin at 1 000.)"""
    c = codec(VBZ_HIP_SEGMENTED=segmented)
    rows, first = pod5_rows(73, [[13, 2049, 5], [13, 2049, 5]])
    frames = [PD.compress_row(x) for x in rows]
    frames[4] = frames[4][: len(frames[4]) // 2]   # the middle row of read 1 cut off
    for bg, en in ((None, None), ([11, 11], [2064, 2064])):
        call = SegCall(c, frames, rows, first, S.DEFAULT, bg, en, failed={1})
        assert call.call() == 0, c.L.vbz_gpu_last_error(c.ctx)
        call.check(row_expect={4: 0xFFFFFFFF})
        assert call.want_first[2] == call.want_first[1] and call.refused == set()
        assert bg is not None or 13 in call.want_st[0].tolist()   # (the planted step on the seam at 13; the range begins too close to it)


# ---- the cap on start[], the count-only call, failed reads -------------------------------------------------------------------------------------
def cap_case(c):
    rng = np.random.default_rng(19)
    return Frames(c, [steps(rng, T) for T in (3000, 0, 700, 5000, 64)], c.options(True, 2, 1, 1))


def test_start_cap_exact_and_one_short():
    c = codec()
    fr = cap_case(c)
    total = int(SegRun(fr).check().want_first[-1])
    r = SegRun(fr, cap=total - 1).check()
    assert r.refused == {4}   # exactly the reads whose rows end beyond the cap
    r = SegRun(fr, cap=int(r.want_first[3])).check()
    assert r.refused == {3, 4}
    r = SegRun(fr, cap=int(r.want_first[1]) - 1).check()
    assert r.refused == {0, 2, 3, 4}   # (read 1 has no sample and no row: nothing to refuse)
    SegRun(fr, cap=total + 9).check()


def test_count_only_call():
    c = codec()
    fr = cap_case(c)
    r = SegRun(fr, count_only=True).check()
    assert r.refused == set() and u32(r.result)[: fr.n].tolist() == [2 * T for T in fr.T]


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
    r = SegRun(fr, failed={2}).check(expect={2: un[2]})
    assert r.want_first[3] == r.want_first[2]
    SegRun(fr, failed={2}, count_only=True).check(expect={2: un[2]})


# ---- the hand-over and the Python methods ------------------------------------------------------------------------------------------------------
def test_hand_over_into_the_event_call():
    """event_first and start go from the segment call straight into signal_events on the device, with the same ranges"""
    c = codec()
    rng = np.random.default_rng(83)
    reads = [steps(rng, T) for T in (0, 9, 2049, 4101, 20_000)]
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    for bg, en in ((None, None), ([3, 1, 7, 2047, 5], [TO_END, 8, 2000, TO_END, 19_000])):
        res = torch.full((fr.n,), -8, dtype=torch.int32, device=c.device)
        first, start = c.signal_segment(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res, fr.opts, begin=bg, end=en)
        mean, sd, n, mom = c.signal_events(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res, fr.opts, first, start, begin=bg, end=en, moments=True)
        torch.cuda.synchronize()
        want_first, st = S.tables(reads, bg, en)
        total = int(want_first[-1])
        assert total > 100 and first.cpu().numpy().tolist() == want_first.tolist()
        want = [EV.event_rows(x, None if bg is None else bg[i], None if en is None else en[i], st[i].tolist(), 0.0, 1.0) for i, x in enumerate(reads)]
        rows, moms = np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want])
        assert (mean.cpu().numpy().view(np.uint32)[:total] == rows[:, 0]).all() and (sd.cpu().numpy().view(np.uint32)[:total] == rows[:, 1]).all()
        assert (n.cpu().numpy().view(np.uint32)[:total] == rows[:, 2]).all() and (mom.cpu().numpy()[:total] == moms).all()
        assert u32(res).tolist() == [2 * T for T in fr.T]


def test_python_methods():
    c = codec()
    dev = c.device
    rng = np.random.default_rng(2)
    reads = [steps(rng, T) for T in (0, 1, 65, 2049, 6151)]
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    res = torch.full((fr.n,), -8, dtype=torch.int32, device=dev)
    sg = batch.Segmentation(3, 6, 4.0, 9.0, 2)
    first, start = c.signal_segment(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res, fr.opts, sg)
    torch.cuda.synchronize()
    want_first, st = S.tables(reads)
    assert first.dtype == torch.int64 and start.dtype == torch.int32 and first.device == dev and start.device == dev
    assert int(start.numel()) == sum(sg.max_rows(T) for T in fr.T) >= int(want_first[-1]) > 100   # (the bound sizes start)
    assert first.cpu().numpy().tolist() == want_first.tolist() and u32(start)[: int(want_first[-1])].tolist() == np.concatenate(st).tolist()
    assert u32(res).tolist() == [2 * T for T in fr.T]
    first0, none = c.signal_segment(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res, fr.opts, sg, start_cap=0)   # the count-only call
    torch.cuda.synchronize()
    assert none is None and first0.cpu().numpy().tolist() == want_first.tolist()
    # POD5
    prow, pfirst = pod5_rows(5, [[13, 7, 1, 2047, 2049], [800, 0, 800], [300] * 10, []])
    src, off, size = arena(c, [PD.compress_row(x) for x in prow], 16)
    res = torch.full((len(prow),), -8, dtype=torch.int32, device=dev)
    rr = torch.full((len(pfirst),), -8, dtype=torch.int32, device=dev)
    first, start, rr2 = c.pod5_signal_segment(src, off, size, i32([len(x) for x in prow]).to(dev), pfirst, res, sg, signed=False, read_result=rr)
    torch.cuda.synchronize()
    sig = [x.view(np.uint16) for x in PR.read_signals(prow, pfirst)]
    want_first, st = S.tables(sig)
    assert first.cpu().numpy().tolist() == want_first.tolist() and u32(start)[: int(want_first[-1])].tolist() == np.concatenate(st).tolist()
    assert want_first[-1] > 100 and u32(rr2).tolist() == [2 * len(x) for x in sig] and u32(res).tolist() == [2 * len(x) for x in prow]
