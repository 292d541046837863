"""The signal trim on the MI355X (include/vbz_gpu.h: vbz_gpu_trim, vbz_gpu_signal_trim_batch, vbz_gpu_pod5_signal_trim_batch).  Every begin[]
entry is held to tests/trim_ref.py, shift_scale bit for bit to norm_ref / ranges_ref, result[] to the statistics call's; the begin table
lies between guard words that must stay untouched.  Sizes around min_trim, a window, a tile and max_samples crossed with the trim's
fields; every option; the large-read path, split and routed call shapes, libzstd's and checksummed frames; POD5 rows and POD5 reads of
several rows; damage, refusals, and the hand-over of begin[] to the range calls without a host copy."""
import ctypes

import numpy as np
import pytest
import torch

import norm_ref as R
import oracle_lib as O
import pod5_ref as P
import pod5_reads_ref as PR
import ranges_ref as G
import trim_ref as T
from trim_support import GUARD_WORD, TrimRun, guarded, table_and_guards, want_begin
from typed_support import NORMS, Call, Frames, arena, codec, full, i32, ranges_struct, trim_struct, u32, unranged_results
from vbz_compression_amd import _lib, batch

pytestmark = pytest.mark.gpu

E_ZSTD, E_INPUT, E_STREAM = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFB
TO_END = 0xFFFFFFFF
SEG = 16_384


def stats_results(fr, norm, signed=True, src=None, size=None):
    """result[] of the statistics call over the same frames"""
    c = fr.c
    res = torch.full((max(fr.n, 1),), -8, dtype=torch.int32, device=c.device)
    c.signal_norm(fr.src if src is None else src, fr.off, fr.size if size is None else size, fr.doff, fr.dcap, res, fr.opts, NORMS[norm][1], signed=signed,
                  sized=fr.sized)
    torch.cuda.synchronize()
    return u32(res)[: fr.n].tolist()


# ---- 1. sizes x the trim's fields -----------------------------------------------------------------------------------------------------------
_grid = {}


def grid(c, signed):
    """the generator's reads over the size list, compressed once: int16 reads, or uint16 ones at a level beyond int16"""
    if signed not in _grid:
        _grid[signed] = Frames(c, T.gpu_reads(level=400 if signed else 40_000), c.options(True, 2, 1, 1))
    return _grid[signed]


def stat_ranges(fr):
    """(stat_begin, stat_end, stats): none; a range inside every read; the read's statistics beside tables; an empty range"""
    inner = ([t // 4 for t in fr.T], [t - t // 8 for t in fr.T])
    return [(None, None, 0), (inner[0], inner[1], 0), (inner[0], None, 1), ([5] * fr.n, [5] * fr.n, 0)]


@pytest.mark.parametrize("signed", [True, False], ids=["int16", "uint16"])
@pytest.mark.parametrize("norm", ["med_mad", "quantile"])
def test_sizes_and_fields(norm, signed):
    c = codec()
    fr = grid(c, signed)
    want_res = stats_results(fr, norm, signed)
    assert want_res == [2 * t for t in fr.T]
    moved = 0
    k = 0
    for W in (1, 7, 40, 64, 4096):
        for m in (0, 3):
            for flags in (0, T.REJECT_AT_END):
                for mf in (1.0, 0.3):
                    sb, se, stats = stat_ranges(fr)[(k + k // 4) % 4]   # (rotating: every flag and fraction meets every kind of statistics range)
                    k += 1
                    p = (W, m, 10, 8000 if W > 1 else 10 + T.MAX_WINDOWS, 2.4, mf, flags)   # (W = 1: as many samples as the window limit takes)
                    run = TrimRun(fr, p, norm, signed, sb, se, stats, with_ss=k % 3 != 0)
                    got = run.check()
                    assert u32(run.result)[: fr.n].tolist() == want_res
                    moved += sum(b not in (0, 10) for b in got)
    for sb, se, stats in stat_ranges(fr):    # the defaults under every kind of statistics range
        got = TrimRun(fr, T.DEFAULT, norm, signed, sb, se, stats).check()
    assert moved > 0


def test_other_min_trim_max_samples_and_factor():
    c = codec()
    fr = grid(c, True)
    for p in ((40, 3, 0, 8000, 2.4, 1.0, 0), (40, 3, 2050, 8000, 2.4, 1.0, 0), (40, 3, 10, 2049, 2.4, 1.0, 1), (40, 3, 9000, 8000, 2.4, 1.0, 0),
              (40, 3, 10, 1, 2.4, 1.0, 0), (33, 2, 7, 100_000, 2.4, 0.3, 0), (40, 3, 10, 8000, -1e30, 1.0, 0), (40, 3, 10, 8000, 1e30, 1.0, 0),
              (40, 39, 10, 8000, 2.4, 1.0, 0), (40, 40, 10, 8000, 2.4, 1.0, 0), (65536, 0, 0, 1 << 28, 0.0, 1.0, 0), (1, 0, 0xFFFFFFFF, 0xFFFFFFFF, 2.4, 1.0, 0)):
        TrimRun(fr, p, "med_mad").check()
    # a norm whose shift overflows to -inf makes every sample high: the peak never comes down
    low = ((R.QUANTILE, 0.2, 0.9, -3e38, 1.0, float("-inf"), 1.0), batch.Normalization("quantile", 0.2, 0.9, -3e38, 1.0, float("-inf"), 1.0))
    with np.errstate(over="ignore"):
        got = TrimRun(fr, T.DEFAULT, low).check()
    assert all(b == min(10, t) for b, t in zip(got, fr.T))


def test_the_window_limit():
    c = codec()
    fr = grid(c, True)
    t0 = 10
    got = TrimRun(fr, (1, 0, t0, t0 + 4096, 2.4, 1.0, 0)).check()      # 4096 windows of one sample: accepted and exact
    assert any(b not in (0, t0) for b in got)
    TrimRun(fr, (1, 3, t0, t0 + 4096, 2.4, 1.0, 0)).check()            # (m >= W: no window can open a peak)
    run = TrimRun(fr, (1, 0, t0, t0 + 4097, 2.4, 1.0, 0))
    assert run.rc == -2 and run.err.decode() != ""
    assert table_and_guards(run.begin, fr.n) == [GUARD_WORD] * fr.n and (run.result.cpu() == -8).all() and (run.ss.cpu() == -777.0).all()
    assert TrimRun(fr, (2, 0, 0, 8194, 2.4, 1.0, 0)).rc == -2 and TrimRun(fr, (2, 0, 0, 8193, 2.4, 1.0, 0)).check()
    TrimRun(fr, (1, 0, 0xFFFFFFF0, 5000, 2.4, 1.0, 0)).check()          # (min_trim beyond max_samples: no window, nothing to refuse)


# ---- 2. options -------------------------------------------------------------------------------------------------------------------------------
OPTION_SIZES = [0, 1, 9, 51, 513, 2049, 4101, 8050, 20_000]


@pytest.mark.parametrize("sized", [False, True], ids=["unsized", "sized"])
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("version", [0, 1])
@pytest.mark.parametrize("zz", [True, False], ids=["zz", "nozz"])
def test_options(zz, version, level, sized):
    c = codec()
    fr = Frames(c, T.gpu_reads(seed=11 + version, sizes=OPTION_SIZES), c.options(zz, 2, level, version), sized, slack=6)
    for norm in ("med_mad", "quantile"):
        run = TrimRun(fr, T.DEFAULT, norm)
        run.check()
        assert u32(run.result)[: fr.n].tolist() == stats_results(fr, norm)
    TrimRun(fr, (7, 0, 3, 5000, 2.4, 0.3, 1), "med_mad", sb=[3] * fr.n, se=[TO_END] * fr.n).check()


# ---- 3. the large-read path ---------------------------------------------------------------------------------------------------------------------
def large_reads():
    """reads of 3 segments and 5 samples: a plateau across the segment boundary at 16 384, one inside the window that straddles it, one
    in front, and one across the second boundary that never comes down before max_samples"""
    rng = np.random.default_rng(31)
    n = 3 * SEG + 5
    out = []
    for a, b in ((16_000, 17_000), (16_375, 16_400), (0, 1500), (2 * SEG - 300, 45_000), (16_383, 16_385)):
        x = T.make_read(rng, n, "none")
        x[a:b] += 150
        out.append(x)
    return out


LARGE_TRIM = (40, 3, 10, 40_000, 2.4, 1.0, 0)    # 999 windows; window 409 is [16 370, 16 410)


def large_read_checks(c):
    seen = []
    for k, x in enumerate(large_reads()):
        fr = Frames(c, [x], c.options(True, 2, 1, 1))
        got = TrimRun(fr, LARGE_TRIM, "med_mad").check()
        seen.append(got[0])
        TrimRun(fr, LARGE_TRIM, "quantile", sb=[SEG - 3], se=[2 * SEG + 1]).check()
        TrimRun(fr, T.DEFAULT, "med_mad").check()                                   # the prefix ends inside the first segment
        TrimRun(fr, (1, 0, SEG - 2000, SEG + 2096, 2.4, 1.0, 0), "med_mad").check()   # 4096 one-sample windows across the boundary
        TrimRun(fr, (4096, 3, 1, 49_157, 2.4, 0.9, 1), "med_mad", signed=False).check()
    assert seen[:3] == [17_010, 16_410, 1530], seen
    assert seen[3] == 10 and seen[4] == 10       # never comes down before max_samples; two high samples open no peak


def test_one_large_read_alone_in_a_call():
    large_read_checks(codec())


@pytest.mark.parametrize("segmented", [1, 0])
def test_large_read_on_forced_paths(segmented):
    large_read_checks(codec(VBZ_HIP_SEGMENTED=segmented))


def test_several_large_reads_in_one_call_on_the_large_read_path():
    c = codec(VBZ_HIP_SEGMENTED=1)
    reads = large_reads() + T.gpu_reads(seed=13, sizes=[0, 9, 2049, 20_000])
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    for norm in ("med_mad", "quantile"):
        TrimRun(fr, LARGE_TRIM, norm).check()
        TrimRun(fr, T.DEFAULT, norm, with_ss=False).check()
    fr0 = Frames(c, reads, c.options(False, 2, 0, 0))     # no zig-zag, level 0
    TrimRun(fr0, LARGE_TRIM, "med_mad").check()


# ---- 4. split and routing -----------------------------------------------------------------------------------------------------------------------
def small_batch(seed, n, lo=50, hi=3000):
    rng = np.random.default_rng(seed)
    return [T.make_read(rng, int(rng.integers(lo, hi)), T.KINDS[i % len(T.KINDS)]) for i in range(n)]


def test_split_batch():
    reads = small_batch(41, 200)
    outs = []
    for c in (codec(VBZ_HIP_SPLIT_MIN=64), codec(VBZ_HIP_SPLIT_MIN=0)):
        fr = Frames(c, reads, c.options(True, 2, 1, 1))
        run = TrimRun(fr, T.DEFAULT, "med_mad")
        got = run.check()
        outs.append((got, run.ss.cpu().numpy().tobytes(), u32(run.result).tolist()))
        TrimRun(fr, (7, 0, 3, 2000, 2.4, 0.3, 1), "quantile", with_ss=False).check()
    assert outs[0] == outs[1]
    assert sum(b not in (0, 10) for b in outs[0][0]) >= 60


def test_routed_long_read_among_small_ones():
    c = codec()
    reads = small_batch(43, 200, 500, 5000)
    rng = np.random.default_rng(44)
    for i, (n, a, b) in {30: (300_000, 0, 2000), 120: (300_000, 16_000, 17_000), 199: (280_001, 5000, 280_001)}.items():
        reads[i] = T.make_read(rng, n, "none")
        reads[i][a:b] += 150
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    got = TrimRun(fr, T.DEFAULT, "med_mad").check()
    assert got[30] == 2010
    got = TrimRun(fr, LARGE_TRIM, "quantile").check()
    assert got[120] == 17_010
    assert u32(TrimRun(fr, T.DEFAULT, "med_mad", with_ss=False).result)[: fr.n].tolist() == stats_results(fr, "med_mad")


def routed_split_reads(at):
    """200 small reads and one of 300 000 samples at index `at`, a plateau at [16 000, 17 000): routed out of a batch that runs as halves"""
    reads = small_batch(45, 200, 500, 5000)
    reads[at] = T.make_read(np.random.default_rng(46), 300_000, "none")
    reads[at][16_000:17_000] += 150
    return reads


def unused_codec(monkeypatch, **env):
    """a context of its own under the knobs.  It has seen no frames, so its first decompress call runs as halves whatever an earlier call
    held (a context that saw mostly frames left to the one-wavefront decoder runs its next call as one group)"""
    for name, v in env.items():
        monkeypatch.setenv(name, str(v))
    c = batch.GpuCodec(0)
    for name in env:
        monkeypatch.delenv(name)
    return c


@pytest.mark.parametrize("at", [30, 150], ids=["lower-half", "upper-half"])
def test_routed_long_read_in_a_split_batch(at, monkeypatch):
    """both cuts of one call: the routed read writes begin and shift_scale through the map, the upper half through its offset tables"""
    reads = routed_split_reads(at)
    outs = []
    # (shape: the call's launches of route and svb_decode -- routed and two halves, the routed group's own not counted; one group)
    for c, shape in ((unused_codec(monkeypatch, VBZ_HIP_SPLIT_MIN=64), (1, 2)), (codec(VBZ_HIP_SPLIT_MIN=64), None),
                     (codec(VBZ_HIP_SPLIT_MIN=0, VBZ_HIP_ROUTING=0), (0, 1))):
        fr = Frames(c, reads, c.options(True, 2, 1, 1))
        c.profile_reset()
        c.profile(True)
        run = TrimRun(fr, LARGE_TRIM, "quantile")
        c.profile(False)
        prof = {k: v[0] for k, v in c.profile_read().items()}
        assert shape is None or (prof.get("route", 0), prof["svb_decode"]) == shape, sorted(prof.items())
        got = run.check()
        assert got[at] >= 17_000, got[at]
        outs.append((got, run.ss.cpu().numpy().tobytes(), u32(run.result).tolist()))
    assert outs[0] == outs[2] and outs[1] == outs[2]


def test_a_trim_call_leaves_nothing_behind_on_its_codec(monkeypatch):
    """a plain decompress and a compress of the same reads behind a trim call that ran routed and as halves (asserted: one route, two
    svb_decode), so that the upper half's and the routed reads' contexts have served it: the bytes of a context that has run no typed
    call.  The trim is the call's, not the context's or its children's.  (Which shape the plain decompress takes is the library's
    choice and not asserted.)"""
    reads = routed_split_reads(150)
    outs = []
    for trim_first in (True, False):
        c = unused_codec(monkeypatch, VBZ_HIP_SPLIT_MIN=64)
        opts = c.options(True, 2, 1, 1)
        fr = Frames(c, reads, opts)
        if trim_first:
            c.profile_reset()
            c.profile(True)
            run = TrimRun(fr, LARGE_TRIM, "quantile")
            c.profile(False)
            prof = {k: v[0] for k, v in c.profile_read().items()}
            assert (prof.get("route", 0), prof["svb_decode"]) == (1, 2), sorted(prof.items())
            run.check()
        back = torch.full((fr.dst_bytes + 64,), 0x5A, dtype=torch.uint8, device=c.device)
        res = torch.full((fr.n,), -8, dtype=torch.int32, device=c.device)
        c.decompress(fr.src, fr.off, fr.size, back, fr.doff, fr.dcap, res, opts)
        again = Frames(c, reads, opts)   # (the compress call)
        torch.cuda.synchronize()
        assert u32(res).tolist() == [2 * t for t in fr.T]
        host = back.cpu().numpy()
        assert all(host[o : o + 2 * t].tobytes() == x.tobytes() for o, t, x in zip(fr.doff.tolist(), fr.T, fr.reads))
        outs.append((host.tobytes(), again.src.cpu().numpy().tobytes(), u32(again.size).tolist()))
    assert outs[0] == outs[1]


# ---- 5. frames of other origins --------------------------------------------------------------------------------------------------------------------
def test_libzstd_frames():
    c = codec()
    reads = T.gpu_reads(seed=51, sizes=[0, 1, 9, 2049, 4101, 50_000])
    comp = arena(c, [O.compress(x, O.options(True, 2, 1, 1), sized=True) for x in reads], 64)
    fr = Frames(c, reads, c.options(True, 2, 1, 1), sized=True, comp=comp)
    TrimRun(fr, T.DEFAULT, "med_mad").check()
    TrimRun(fr, (64, 3, 10, 8000, 2.4, 0.3, 1), "quantile").check()


def test_checksummed_frames():
    c = codec()
    reads = T.gpu_reads(seed=52, sizes=[0, 1, 9, 2049, 4101, 50_000])
    c.set_checksum(1)
    try:
        fr = Frames(c, reads, c.options(True, 2, 1, 1))
    finally:
        c.set_checksum(0)
    TrimRun(fr, T.DEFAULT, "quantile").check()
    TrimRun(fr, (7, 0, 10, 8000, 2.4, 1.0, 0), "med_mad").check()


# ---- 6. POD5 -------------------------------------------------------------------------------------------------------------------------------------
def test_pod5_rows_as_reads_of_their_own():
    c = codec()
    rows = T.gpu_reads(seed=61)
    fr = Frames(c, rows, batch.pod5_options(), comp=arena(c, [P.compress_row(x) for x in rows], 64))
    for norm in ("med_mad", "quantile"):
        run = TrimRun(fr, T.DEFAULT, norm)
        run.check()
        assert u32(run.result)[: fr.n].tolist() == stats_results(fr, norm)
    TrimRun(fr, (7, 0, 3, 5000, 2.4, 0.3, 1), "med_mad", signed=False, sb=[3] * fr.n, se=[TO_END] * fr.n).check()
    TrimRun(fr, (1, 0, 10, 4106, 2.4, 1.0, 0), "med_mad", with_ss=False).check()


# rows per read: ends inside a window; ends inside the min_trim prefix; empty rows; no rows; 200 short rows; a first row longer than
# max_samples; one row; rows of whole tiles
POD5_SHAPES = [[147, 23, 1, 2000, 3000], [4, 3, 2, 1, 3000], [0, 500, 0, 0, 1500, 0], [], [25] * 200, [9000, 500], [6000], [2048, 2048, 4096, 5], [0, 0], [3, 4]]


def pod5_case(seed=71, shapes=POD5_SHAPES, kinds=T.KINDS):
    rng = np.random.default_rng(seed)
    rows, first = [], []
    for k, lens in enumerate(shapes):
        x = T.make_read(rng, sum(lens), kinds[k % len(kinds)])
        first.append(len(rows))
        at = 0
        for n in lens:
            rows.append(x[at : at + n])
            at += n
    return rows, first, [P.compress_row(x) for x in rows]


class TrimCall(Call):
    """Call with a guarded begin table: the raw vbz_gpu_pod5_signal_trim_batch call"""

    def __init__(self, c, frames, rows, first, norm, table=None):
        super().__init__(c, frames, [len(x) for x in rows], PR.bounds(first, len(rows)) if table is None else table, norm=norm)
        self.begin, self.begin_ptr = guarded(c, self.R)

    def trim_call(self, p, sb=None, se=None, stats=0, signed=True, with_ss=True):
        g, self.gkeep = ranges_struct(self.c, sb, se, stats)
        t = trim_struct(p)
        rc = self.c.L.vbz_gpu_pod5_signal_trim_batch(self.c.ctx, ctypes.byref(self.b), ctypes.byref(self.opts), int(signed), ctypes.byref(self.reads),
                                                     ctypes.byref(self.m), ctypes.byref(g) if (sb is not None or se is not None) else None,
                                                     ctypes.byref(t), self.ss.data_ptr() if with_ss else None, self.begin_ptr)
        self.c.synchronize()
        return rc


def check_pod5(call, rows, first, norm, p, sb=None, se=None, stats=0, signed=True, failed=(), with_ss=True):
    got = table_and_guards(call.begin, call.R)
    ss = call.ss.cpu().numpy()
    sbs, ses = full(sb, call.R), full(se, call.R)
    for k, x in enumerate(PR.read_signals(rows, first)):
        if k in failed:
            assert got[k] == 0, ("begin of a failed read", k, got[k])
            continue
        want, shift, scale = want_begin(x if signed else x.view(np.uint16), norm, p, sbs[k], ses[k], stats)
        assert got[k] == want, ("begin", k, len(x), p, got[k], want)
        if with_ss:
            assert (ss[k][0].view(np.uint32), ss[k][1].view(np.uint32)) == (shift.view(np.uint32), scale.view(np.uint32)), ("shift_scale", k)
    return got


@pytest.mark.parametrize("segmented", [0, 1])
def test_pod5_reads(segmented):
    c = codec(VBZ_HIP_SEGMENTED=segmented)
    rows, first, frames = pod5_case()
    Ts = [len(x) for x in PR.read_signals(rows, first)]
    moved = 0
    for name, (ref, nm) in NORMS.items():
        want = unranged_results(c, frames, rows, first, None, nm)
        for p in (T.DEFAULT, (40, 3, 10, 8000, 2.4, 0.3, 1), (7, 0, 3, 5000, 2.4, 1.0, 0), (1, 0, 140, 4236, 2.4, 1.0, 0), (64, 3, 10, 100_000, 2.4, 1.0, 0)):
            call = TrimCall(c, frames, rows, first, nm)
            assert call.trim_call(p) == 0, c.L.vbz_gpu_last_error(c.ctx)
            assert (u32(call.result)[: call.n].tolist(), u32(call.read_result)[: call.R].tolist()) == want
            moved += sum(b not in (0, p[2]) for b in check_pod5(call, rows, first, ref, p))
        sb, se = [t // 4 for t in Ts], [t - t // 8 for t in Ts]
        for stats in (0, 1):
            call = TrimCall(c, frames, rows, first, nm)
            assert call.trim_call(T.DEFAULT, sb, se, stats) == 0
            check_pod5(call, rows, first, ref, T.DEFAULT, sb, se, stats)
        call = TrimCall(c, frames, rows, first, nm)
        assert call.trim_call(T.DEFAULT, signed=False, with_ss=False) == 0
        check_pod5(call, rows, first, ref, T.DEFAULT, signed=False, with_ss=False)
        assert (call.ss.cpu().numpy() == -777.0).all()
    assert moved >= 10


def test_pod5_reads_split_shape():
    rng = np.random.default_rng(81)
    shapes = [[int(v) for v in rng.integers(0, 900, int(rng.integers(1, 6)))] for _ in range(70)]
    rows, first, frames = pod5_case(81, shapes)
    outs = []
    for c in (codec(VBZ_HIP_SPLIT_MIN=64), codec(VBZ_HIP_SPLIT_MIN=0)):
        call = TrimCall(c, frames, rows, first, batch.MED_MAD)
        assert call.trim_call(T.DEFAULT) == 0
        outs.append(check_pod5(call, rows, first, R.BONITO, T.DEFAULT))
    assert outs[0] == outs[1]


# ---- 7. damage --------------------------------------------------------------------------------------------------------------------------------------
def test_damage_behind_the_prefix_keeps_its_verdict_and_gives_zero():
    c = codec()
    rng = np.random.default_rng(92)
    reads = [T.make_read(rng, 12_000, "front") for _ in range(6)]
    opts = c.options(True, 2, 0, 1)   # (level 0: the svb stream itself, so the damage is the stream's)
    fr = Frames(c, reads, opts)
    src = fr.src.clone()
    offs, sizes = fr.off.cpu().numpy(), u32(fr.size)
    size = fr.size.clone()
    size[3] = int(sizes[3]) - 5                        # a stream cut short, far behind max_samples
    src[int(offs[4]) + 12_000 // 4 - 3] = 0xFF         # control bytes of the last samples announce more bytes than there are
    un = stats_results(fr, "med_mad", src=src, size=size)
    assert un[3] == E_STREAM and _lib.is_error(un[4]) and un[1] == 24_000
    expect = {i: v for i, v in enumerate(un) if _lib.is_error(v)}
    got = TrimRun(fr, T.DEFAULT, "med_mad", src=src, size=size).check(expect=expect)
    assert got[3] == 0 and got[4] == 0 and all(got[i] > 10 for i in (0, 1, 2, 5))
    # a zstd frame damaged in its middle: whatever the statistics call says of it
    fr2 = Frames(c, reads[:3], c.options(True, 2, 1, 1))
    src2 = fr2.src.clone()
    o2, s2 = fr2.off.cpu().numpy(), u32(fr2.size)
    src2[int(o2[1]) + int(s2[1]) // 2 : int(o2[1]) + int(s2[1]) // 2 + 4] ^= 0x5A
    un2 = stats_results(fr2, "med_mad", src=src2)
    if _lib.is_error(un2[1]):     # (a change the decoder cannot notice leaves other samples: nothing to hold them to)
        TrimRun(fr2, T.DEFAULT, "med_mad", src=src2).check(expect={1: un2[1]})


def test_pod5_row_failing_inside_a_read():
    c = codec()
    shapes = [[600, 700], [900, 1000, 1100], [500], [900, 1000, 9100], [640]]
    rows, first, good = pod5_case(21, shapes, kinds=("front",))
    frames = list(good)
    frames[3] = good[3][: len(good[3]) // 2]                       # a damaged frame in the middle row of read 1
    frames[7] = O.zstd_compress(P.svb16_encode(rows[7])[:-1], 1)   # a stream with a byte cut off in the middle row of read 3
    want = unranged_results(c, frames, rows, first, None, batch.MED_MAD)
    assert want[0][3] == E_ZSTD and want[0][7] == E_STREAM
    call = TrimCall(c, frames, rows, first, batch.MED_MAD)
    assert call.trim_call(T.DEFAULT) == 0
    assert (u32(call.result)[: call.n].tolist(), u32(call.read_result)[: call.R].tolist()) == want
    got = check_pod5(call, rows, first, R.BONITO, T.DEFAULT, failed=(1, 3), with_ss=False)
    assert got[0] > 10 and got[2] > 10 and got[4] > 10


@pytest.mark.parametrize("table", [[1, 2, 5, 6, 9, 10], [0, 2, 5, 4, 9, 10], [0, 2, 5, 6, 9, 11]], ids=["first-not-0", "decreasing", "last-not-n"])
def test_bad_first_row_fails_whole(table):
    c = codec()
    shapes = [[600, 700], [900, 1000, 1100], [500], [900, 1000, 1100], [640]]
    rows, first, frames = pod5_case(22, shapes)
    call = TrimCall(c, frames, rows, first, batch.MED_MAD, table=table)
    assert call.trim_call(T.DEFAULT) == 0
    assert u32(call.result)[: call.n].tolist() == [E_INPUT] * call.n and u32(call.read_result)[: call.R].tolist() == [E_INPUT] * call.R
    assert table_and_guards(call.begin, call.R) == [GUARD_WORD] * call.R, "begin was written under a bad first_row"
    assert (call.ss.cpu().numpy() == -777.0).all()


# ---- 8. the hand-over ------------------------------------------------------------------------------------------------------------------------------
def test_begin_feeds_the_range_calls_without_a_host_copy():
    c = codec()
    reads = T.gpu_reads(seed=95, sizes=[0, 9, 513, 2049, 4101, 8050, 20_000])
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    samples = i32(fr.T).to(c.device)
    L, S, mode, ea, pad = 1024, 1000, "end", 6, -7.0
    res = torch.full((fr.n,), -8, dtype=torch.int32, device=c.device)
    # Bonito's order: trim by the whole read's statistics, then normalise and chunk signal[trim:]
    begin, ss = c.signal_trim(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res, fr.opts, batch.MED_MAD, shift_scale=True)
    assert begin.device == c.device and begin.dtype == torch.int32
    res2 = torch.full((fr.n,), -8, dtype=torch.int32, device=c.device)
    ch, cf, info = c.decompress_chunks(fr.src, fr.off, fr.size, samples, res2, fr.opts, L, S, mode=mode, end_align=ea, pad=pad, norm=batch.MED_MAD, begin=begin)
    # Dorado's order: normalise by the whole read, drop signal[:trim]; the constants of the trim call as given constants
    offset = -ss[:, 0].contiguous()
    scale = (1.0 / ss[:, 1].double()).float().contiguous()
    res3 = torch.full((fr.n,), -8, dtype=torch.int32, device=c.device)
    ch3, cf3, info3 = c.decompress_chunks(fr.src, fr.off, fr.size, samples, res3, fr.opts, L, S, mode=mode, end_align=ea, pad=pad, offset=offset, scale=scale,
                                          begin=begin)
    res4 = torch.full((fr.n,), -8, dtype=torch.int32, device=c.device)
    ch4, cf4, _ = c.decompress_chunks(fr.src, fr.off, fr.size, samples, res4, fr.opts, L, S, mode=mode, end_align=ea, pad=pad, norm=batch.MED_MAD, begin=begin,
                                      stats="read")
    torch.cuda.synchronize()
    got_begin = u32(begin).tolist()
    cf, cf3 = cf.cpu().numpy(), cf3.cpu().numpy()
    bits, bits3 = ch.view(torch.int16).cpu().numpy().view(np.uint16), ch3.view(torch.int16).cpu().numpy().view(np.uint16)
    assert u32(res).tolist() == u32(res2).tolist() == u32(res3).tolist() == [2 * t for t in fr.T]
    want_info = []
    for i, x in enumerate(fr.reads):
        b = T.begin(x, R.BONITO)
        assert got_begin[i] == b, (i, got_begin[i], b)
        starts, want, _, _ = G.norm_chunk_rows(x, b, None, L, S, mode, ea, R.BONITO, G.STATS_RANGE, pad, "f16")
        assert cf[i + 1] - cf[i] == len(starts) and (bits[cf[i] : cf[i + 1]] == want).all(), ("trim, then normalise", i)
        starts, want, _, _ = G.norm_chunk_rows(x, b, None, L, S, mode, ea, R.BONITO, G.STATS_READ, pad, "f16")
        assert cf3[i + 1] - cf3[i] == len(starts) and (bits3[cf3[i] : cf3[i + 1]] == want).all(), ("given constants", i)
        want_info += [[i, int(s)] for s in starts]
    assert info3.cpu().numpy().tolist() == want_info
    assert ch4.view(torch.int16).cpu().numpy().tobytes() == ch3.view(torch.int16).cpu().numpy().tobytes() and cf4.cpu().numpy().tolist() == cf3.tolist()
    assert sum(b not in (0, 10) for b in got_begin) >= 10


def test_pod5_begin_feeds_the_pod5_range_call():
    c = codec()
    rows, first, frames = pod5_case()
    src, off, size = arena(c, frames, 16)
    rs = i32([len(x) for x in rows]).to(c.device)
    res = torch.full((len(rows),), -8, dtype=torch.int32, device=c.device)
    begin, ss, rr = c.pod5_signal_trim(src, off, size, rs, first, res, batch.MED_MAD, shift_scale=True)
    res2 = torch.full((len(rows),), -8, dtype=torch.int32, device=c.device)
    ch, cf, info, rr2 = c.pod5_decompress_chunks(src, off, size, rs, first, res2, 1024, 1000, mode="end", end_align=6, pad=-7.0, norm=batch.MED_MAD, begin=begin)
    torch.cuda.synchronize()
    sig = PR.read_signals(rows, first)
    assert u32(begin).tolist() == T.pod5_begins(rows, first, R.BONITO)
    assert u32(rr).tolist() == u32(rr2).tolist() == [2 * len(x) for x in sig]
    cf = cf.cpu().numpy()
    bits = ch.view(torch.int16).cpu().numpy().view(np.uint16)
    ssh = ss.cpu().numpy()
    for k, x in enumerate(sig):
        b = T.begin(x, R.BONITO)
        starts, want, _, _ = G.norm_chunk_rows(x, b, None, 1024, 1000, "end", 6, R.BONITO, G.STATS_RANGE, -7.0, "f16")
        assert cf[k + 1] - cf[k] == len(starts) and (bits[cf[k] : cf[k + 1]] == want).all(), k
        shift, scale = R.shift_scale(x, R.BONITO)
        assert (ssh[k][0].view(np.uint32), ssh[k][1].view(np.uint32)) == (shift.view(np.uint32), scale.view(np.uint32)), k


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_host_refusals_launch_nothing():
    c = codec()
    L = c.L
    fr = Frames(c, small_batch(93, 4, 400, 600), c.options(True, 2, 1, 1))
    n = fr.n
    res = torch.full((n,), 12345, dtype=torch.int32, device=c.device)
    ss = torch.full((n, 2), 7.0, dtype=torch.float32, device=c.device)
    begin, ptr = guarded(c, n)
    b = c._batch(fr.src, fr.off, fr.size, torch.empty(0, dtype=torch.uint8, device=c.device), fr.doff, fr.dcap, res)
    b.dst, b.dst_bytes = None, fr.dst_bytes
    m = batch.MED_MAD.c_struct()
    rows, first, frames = pod5_case(22, [[600, 700], [900, 1000, 1100], [500, 20]])
    pc = TrimCall(c, frames, rows, first, batch.MED_MAD)

    def calls(t, o=fr.opts, mp=m, g=None, bp=ptr, pbp=None, ssp=ss.data_ptr(), po=None, which=(0, 1)):
        tp = ctypes.byref(t) if t is not None else None
        gp = ctypes.byref(g) if g is not None else None
        fns = [lambda: L.vbz_gpu_signal_trim_batch(c.ctx, ctypes.byref(b), ctypes.byref(o), 0, 1, ctypes.byref(mp), gp, tp, ssp, bp),
               lambda: L.vbz_gpu_pod5_signal_trim_batch(c.ctx, ctypes.byref(pc.b), ctypes.byref(pc.opts if po is None else po), 1, ctypes.byref(pc.reads),
                                                        ctypes.byref(mp), gp, tp, pc.ss.data_ptr(), pc.begin_ptr if pbp is None else pbp)]
        return [fns[k]() for k in which]

    nan, inf = float("nan"), float("inf")
    bad = [(0, 3, 10, 8000, 2.4, 1.0, 0), (65537, 3, 10, 8000, 2.4, 1.0, 0), (40, 3, 10, 0, 2.4, 1.0, 0), (40, 3, 10, 8000, nan, 1.0, 0),
           (40, 3, 10, 8000, inf, 1.0, 0), (40, 3, 10, 8000, -inf, 1.0, 0), (40, 3, 10, 8000, 2.4, 0.0, 0), (40, 3, 10, 8000, 2.4, -0.5, 0),
           (40, 3, 10, 8000, 2.4, 1.0000001, 0), (40, 3, 10, 8000, 2.4, nan, 0), (40, 3, 10, 8000, 2.4, inf, 0), (40, 3, 10, 8000, 2.4, 1.0, 2),
           (40, 3, 10, 8000, 2.4, 1.0, 0x80000001), (1, 3, 10, 4107, 2.4, 1.0, 0), (40, 3, 0, 163_880, 2.4, 1.0, 0), (1, 0, 0, 0xFFFFFFFF, 2.4, 1.0, 0)]
    for p in bad:
        assert calls(trim_struct(p)) == [-2, -2], p
        assert L.vbz_gpu_last_error(c.ctx).decode() != ""
    ok = trim_struct(T.DEFAULT)
    assert calls(trim_struct(T.DEFAULT, reserved=1)) == [-2, -2]
    assert calls(None) == [-2, -2]                                  # a NULL trim
    assert calls(ok, bp=None, pbp=0) == [-2, -2]                    # a NULL begin
    # everything the statistics call refuses
    assert calls(ok, o=_lib.CompressionOptions(True, 4, 1, 1), which=(0,)) == [-2]
    assert calls(ok, po=_lib.CompressionOptions(True, 2, 1, 1), which=(1,)) == [-2]     # the call over POD5 reads takes POD5 options only
    bad_m = batch.MED_MAD.c_struct()
    bad_m.method = 9
    assert calls(ok, mp=bad_m) == [-2, -2]
    for kw in ({"reserved": 1}, {"stats": 2}):
        g, keep = ranges_struct(c, [0] * 4, None, **kw)
        assert calls(ok, g=g) == [-2, -2], kw
    assert L.vbz_gpu_signal_trim_batch(None, ctypes.byref(b), ctypes.byref(fr.opts), 0, 1, ctypes.byref(m), None, ctypes.byref(ok), None, ptr) == -1
    assert L.vbz_gpu_signal_trim_batch(c.ctx, None, ctypes.byref(fr.opts), 0, 1, ctypes.byref(m), None, ctypes.byref(ok), None, ptr) == -1
    torch.cuda.synchronize()
    assert (res.cpu() == 12345).all() and (ss.cpu() == 7.0).all() and table_and_guards(begin, n) == [GUARD_WORD] * n
    assert table_and_guards(pc.begin, pc.R) == [GUARD_WORD] * pc.R and (pc.ss.cpu().numpy() == -777.0).all() and (pc.result.cpu() == -8).all()
    # ... and the accepted edges beside them: a NULL shift_scale, a NULL ranges, the largest window count
    assert calls(trim_struct((40, 3, 0, 163_879, 2.4, 1.0, 0)), ssp=None) == [0, 0]
    c.synchronize()
    assert table_and_guards(begin, n) != [GUARD_WORD] * n and (ss.cpu() == 7.0).all()
