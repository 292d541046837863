"""Signal match on the MI355X (include/vbz_gpu.h: vbz_gpu_match and the three *_match_batch calls).  The stage entry runs match_ref's
catalogue -- every reference length around a lane's last row, the last lane and every change of rows per lane, against query lengths
around the 64-sample load seam and shorter than the pipeline, planted answers, extremes, refused lengths -- every hit bit for bit.  The
fused calls are held to the statement applied to the numpy-decoded signal: the query arena bit for bit against windows_ref, the hits
against match_ref over that query, canaries and guard rows around every arena: codec versions, levels, sized and unsized, both
signednesses, given constants and both normalisations, ranges with an odd begin, T' < N and T' = 0, a split call, the large-read route,
POD5 rows and reads."""
import numpy as np
import pytest
import torch

import match_ref as M
import norm_ref as R
from ranges_ref import pod5_signals
from match_support import EMPTY, MatchCall, MatchRun, assert_hits, query_rows, stage
from typed_support import NORMS, Frames, arena, codec, expect_results, frames_of, i32, sine_signal, u32
from vbz_compression_amd import batch

pytestmark = pytest.mark.gpu

TO_END = 0xFFFFFFFF
O, S = -330.0, 1.0 / 45.0   # given constants that bring sine_signal to about unit scale


# ---- 1. the stage entry over the catalogue ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(M.catalogue())), ids=[c.name for c in M.catalogue()])
def test_stage_entry_catalogue(index):
    call = M.catalogue()[index]
    got = stage(codec(), call)
    want = M.expected(index)
    for (read, ref), hit in call.planted.items():
        assert tuple(int(v) for v in got[read][ref]) == hit, (call.name, "planted", read, ref, got[read][ref].tolist(), hit)
    assert_hits(got, want, call.name)
    refused = [r for r, m in enumerate(call.ref_len) if m == 0 or m > call.stride]
    for r in refused:
        assert (got[:, r] == np.array(EMPTY, np.uint32)).all(), (call.name, "refused column", r)


def test_python_method_and_quantize_levels():
    c = codec()
    rng = np.random.default_rng(5)
    z = rng.normal(0, 1.2, (7, 256)).astype(np.float32)
    ref = np.zeros((3, 64), np.int8)
    ref[0, :40] = batch.quantize_levels(z[2, 100:140], 32.0)   # a stretch of read 2 itself
    ref[1, :64] = rng.integers(-60, 61, 64)
    ref[2, :9] = rng.integers(-128, 128, 9)
    lens = [40, 64, 9]
    valid = [256, 255, 256, 17, 0, 300, 64]
    hits = c.match(torch.from_numpy(z).to(c.device), i32(valid).to(c.device), torch.from_numpy(ref).to(c.device), i32(lens).to(c.device))
    torch.cuda.synchronize()
    got = hits.cpu().numpy().view(np.uint32)
    assert tuple(got.shape) == (7, 3, 2)
    assert_hits(got, M.hits(z, valid, 32.0, ref, lens), "method")
    assert got[2][0].tolist()[0] == 0 and got[2][0].tolist()[1] <= 140 and got[4].tolist() == [EMPTY] * 3


# ---- 2. the fused call ----------------------------------------------------------------------------------------------------------------------
def long_reads(valid, N):
    """the reads whose query holds both planted stretches"""
    return [i for i, v in enumerate(valid) if v >= min(N, 320)]


def refs_for(want_q, valid, quant, rng, stride=416):
    """references for reads whose queries are want_q (bits): stretches of two of the queries themselves (cost 0 there), noise of M = 400
    and 33, one full-range row, and refused lengths"""
    z = want_q.view(np.float32)
    ref = np.zeros((7, stride), np.int8)
    lens = []
    N = z.shape[1]
    long = long_reads(valid, N)
    for r, i in enumerate((long[0], long[-1])):
        at = 37 + 64 * r
        k = M.quantize(z[i, at : at + min(150 + 61 * r, N // 2)], quant)
        ref[r, : len(k)] = k
        lens.append(len(k))
    ref[2, :400] = np.clip(np.repeat(rng.integers(-70, 71, 67), 6)[:400] + rng.integers(-6, 7, 400), -127, 127)
    ref[3, :33] = rng.integers(-50, 51, 33)
    ref[4, :stride] = rng.integers(-128, 128, stride)
    ref[5, :20] = 5
    ref[6, :20] = 5
    return ref, lens + [400, 33, stride, 0, stride + 1]


def run_fused(fr, N, rng, **kw):
    """one fused call over fr, its references cut from the expected queries; the planted columns must find their stretch"""
    n = fr.n
    signed = kw.get("signed", True)
    sig = [x if signed else x.view(np.uint16) for x in fr.reads]
    bg, en = kw.get("begin") or [None] * n, kw.get("end") or [None] * n
    o = kw.get("offset") if kw.get("offset") is not None else np.zeros(n, np.float32)
    s = kw.get("scale") if kw.get("scale") is not None else np.ones(n, np.float32)
    norm = kw.get("norm")
    want_q, _, Tp = query_rows(sig, bg, en, N, list(zip(o, s)), norm[0] if norm else None, kw.get("stats", 0))
    valid = [min(t, N) for t in Tp]
    ref, lens = refs_for(want_q, valid, 32.0, rng)
    run = MatchRun(fr, ref, lens, N, 32.0, **kw).check()
    long = long_reads(valid, N)
    assert int(run.want[long[0]][0][0]) == 0 and int(run.want[long[-1]][1][0]) == 0, "the planted stretches cost nothing"
    return run


SIZES = [0, 1, 7, 9, 513, 2049, 4101, 20_000]


@pytest.mark.parametrize("sized", [False, True], ids=["unsized", "sized"])
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("version", [0, 1])
def test_options_and_signedness(version, level, sized):
    c = codec()
    rng = np.random.default_rng(version * 4 + level * 2 + sized)
    reads = [sine_signal(rng, T) for T in SIZES]
    fr = Frames(c, reads, c.options(True, 2, level, version), sized, slack=6)
    o, s = np.full(fr.n, O, np.float32), np.full(fr.n, S, np.float32)
    run_fused(fr, 1024, rng, offset=o, scale=s)                       # T' < N, T' = 0, T' > N
    run_fused(fr, 1024, rng, signed=False, offset=o, scale=s)


@pytest.mark.parametrize("stats", [0, 1], ids=["range", "read"])
@pytest.mark.parametrize("method", ["med_mad", "quantile"])
def test_normalised_and_ranged(method, stats):
    c = codec()
    rng = np.random.default_rng(29 + stats)
    reads, bg, en = [], [], []
    for T in (0, 1, 9, 513, 2049, 4101, 20_000):
        x = sine_signal(rng, T)
        for b, e in ((3, TO_END), (8, T - 3 if T > 3 else T), (2001, 2600), (TO_END, 0), (0, T)):
            reads.append(x)
            bg.append(b)
            en.append(e)
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    run_fused(fr, 1024, rng, begin=bg, end=en, norm=NORMS[method], stats=stats)
    run_fused(fr, 512, rng, norm=NORMS[method], stats=stats, signed=False)   # (no ranges: the whole read either way)
    run_fused(fr, 1024, rng, begin=bg, offset=np.full(fr.n, O, np.float32), scale=np.full(fr.n, S, np.float32))   # (given constants, odd begins)


def test_split_call():
    rng = np.random.default_rng(31)
    reads = [sine_signal(rng, int(rng.integers(50, 3000))) for _ in range(200)]
    outs = []
    for c in (codec(VBZ_HIP_SPLIT_MIN=64), codec(VBZ_HIP_SPLIT_MIN=0)):
        fr = Frames(c, reads, c.options(True, 2, 1, 1))
        r = run_fused(fr, 256, np.random.default_rng(32), norm=NORMS["med_mad"], begin=[3] * fr.n)
        outs.append((r.a.out.cpu().numpy().tobytes(), r.a.query.cpu().numpy().tobytes()))
    assert outs[0] == outs[1]


@pytest.mark.parametrize("segmented", [None, 1], ids=["by-shape", "forced"])
def test_large_read_route(segmented):
    c = codec() if segmented is None else codec(VBZ_HIP_SEGMENTED=segmented)
    rng = np.random.default_rng(23)
    x = sine_signal(rng, 270_000)
    fr = Frames(c, [x], c.options(True, 2, 1, 1))
    run_fused(fr, 2048, rng, norm=NORMS["med_mad"])
    run_fused(fr, 2048, rng, begin=[16_381], end=[TO_END], offset=[O], scale=[S])


def test_routed_long_read_among_small_ones():
    c = codec()
    rng = np.random.default_rng(41)
    reads = [sine_signal(rng, int(rng.integers(500, 5000))) for _ in range(600)]
    reads[100] = sine_signal(rng, 300_000)
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    run_fused(fr, 512, rng, norm=NORMS["quantile"], begin=[3 if i % 2 else 8 for i in range(fr.n)])


# ---- 3. POD5 ----------------------------------------------------------------------------------------------------------------------------------
POD5_SHAPES = [[1500], [13, 7, 1, 2047, 2049], [800, 0, 800], [24, 8, 2056, 16], [300] * 40, [], [0, 0], [2048, 100]]


def pod5_refs(sig, bg, en, N, consts, norm, stats, rng):
    want_q, _, Tp = query_rows(sig, bg, en, N, consts, norm, stats)
    return refs_for(want_q, [min(t, N) for t in Tp], 32.0, rng)


@pytest.mark.parametrize("segmented", [0, 1])
def test_pod5_reads(segmented):
    c = codec(VBZ_HIP_SEGMENTED=segmented)
    rows, first, frames = frames_of(71, POD5_SHAPES)
    n = len(first)
    rng = np.random.default_rng(3)
    o, s = np.full(n, O, np.float32), np.full(n, S, np.float32)
    consts = list(zip(o, s))
    sig = pod5_signals(rows, first)
    ref, lens = pod5_refs(sig, [None] * n, [None] * n, 1024, consts, None, 0, rng)
    call = MatchCall(c, frames, rows, first, ref, lens, 1024, offset=o, scale=s)
    assert call.call() == 0, c.L.vbz_gpu_last_error(c.ctx)
    expect_results(call, rows, first, 4)
    call.check(consts=consts)
    bg, en = [3, 8, 3, 2000, 701, TO_END, 0, 5], [TO_END, 3000, 1000, 2100, TO_END, 0, TO_END, 2100]
    for stats in (0, 1):
        ref, lens = pod5_refs(sig, bg, en, 512, None, R.BONITO, stats, rng)
        call = MatchCall(c, frames, rows, first, ref, lens, 512, begin=bg, end=en, norm=batch.MED_MAD, stats=stats)
        assert call.call(read_result=stats == 0) == 0, c.L.vbz_gpu_last_error(c.ctx)   # (stats 1: the caller takes no read_result)
        call.check(norm=R.BONITO)


def test_pod5_rows_as_reads_of_their_own_and_the_method():
    c = codec()
    lens = [0, 1, 9, 513, 2049, 4101]
    rows, first, frames = frames_of(73, [[n] for n in lens])
    fr = Frames(c, rows, batch.pod5_options(), comp=arena(c, frames, 64))
    rng = np.random.default_rng(7)
    run_fused(fr, 1024, rng, norm=NORMS["med_mad"], begin=[3] * fr.n)
    # the python methods: the same hits through signal_match and pod5_signal_match
    dev = c.device
    src, off, size = arena(c, frames, 16)
    want_q, _, Tp = query_rows(rows, [None] * 6, [None] * 6, 256, [(O, S)] * 6)
    ref, rl = refs_for(want_q, [min(t, 256) for t in Tp], 32.0, rng)
    ref_d, len_d = torch.from_numpy(ref).to(dev), i32(rl).to(dev)
    od, sd = torch.full((6,), O, dtype=torch.float32, device=dev), torch.full((6,), S, dtype=torch.float32, device=dev)
    res = torch.full((6,), -8, dtype=torch.int32, device=dev)
    hits, query = c.pod5_signal_match(src, off, size, i32(lens).to(dev), list(range(6)), res, ref_d, len_d, batch.Match(256, 32.0), scale=sd, offset=od)
    res2 = torch.full((6,), -8, dtype=torch.int32, device=dev)
    hits2, query2 = c.signal_match(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res2, fr.opts, ref_d, len_d, batch.Match(256, 32.0), scale=sd, offset=od)
    torch.cuda.synchronize()
    want = M.hits(want_q.view(np.float32), [min(t, 256) for t in Tp], 32.0, ref, rl)
    for h, q, r in ((hits, query, res), (hits2, query2, res2)):
        assert (q.cpu().numpy().view(np.uint32) == want_q).all()
        assert_hits(h.cpu().numpy().view(np.uint32), want, "method")
        assert u32(r).tolist() == [4 * t for t in lens]
