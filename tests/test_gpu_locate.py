"""Signal locate on the MI355X (include/vbz_gpu.h: vbz_gpu_locate and the three *_locate_batch calls).  The stage entry runs locate_ref's
catalogue -- every query length around each change of rows per lane, a lane's last row and the last lane, against target lengths on each
side of the loader's block and shorter than the pipeline, planted answers, extremes, refused lengths, one target beyond 65 536 levels --
and a dense sweep of every n against every L up to 136, every hit bit for bit.  The same cells through vbz_gpu_match_batch with the
roles swapped must give the same hits.  The fused calls are held to the statement applied to the numpy-decoded signal: the query arena bit
for bit against windows_ref, the hits against locate_ref over that query, canaries and guard rows around every arena."""
import numpy as np
import pytest
import torch

import locate_ref as LR
import norm_ref as R
from ranges_ref import pod5_signals
from locate_support import LocateCall, LocateRun, stage, stage_arrays, swapped_match
from match_support import EMPTY, assert_hits, query_rows
from typed_support import NORMS, Frames, arena, codec, expect_results, frames_of, i32, sine_signal, u32
from vbz_compression_amd import _lib, batch

pytestmark = pytest.mark.gpu

TO_END = 0xFFFFFFFF
O, S = -330.0, 1.0 / 45.0   # given constants that bring sine_signal to about unit scale
CATALOGUE = LR.catalogue()


# ---- 1. the stage entry ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(CATALOGUE)), ids=[c.name for c in CATALOGUE])
def test_stage_entry_catalogue(index):
    call = CATALOGUE[index]
    got = stage(codec(), call)
    for (read, tg), hit in call.planted.items():
        assert tuple(int(v) for v in got[read][tg]) == hit, (call.name, "planted", read, tg, got[read][tg].tolist(), hit)
    assert_hits(got, LR.expected(index), call.name)
    refused = [g for g, L in enumerate(call.target_len) if L == 0 or L > call.stride]
    for g in refused:
        assert (got[:, g] == np.array(EMPTY, np.uint32)).all(), (call.name, "refused column", g)


def test_dense_sweep():
    """every n = 1 ... 136 against every L = 1 ... 136 in one call: NaN, infinities and +-1e30 behind every read's end, random int8 with -128
    behind every target's end"""
    query, valid, target, target_len, want = LR.sweep()
    assert query.shape == (136, 136) and target.shape == (136, 144)
    assert not (np.abs(query[0, 1:]) < 1e29).any() and np.isnan(query[0, 1:]).any() and (target[:, 136:] == -128).any()
    got = stage_arrays(codec(), query, valid, 32.0, target, target_len)
    assert_hits(got, want, "sweep")


def test_one_read_per_rows_per_lane():
    """a read from the upper half of each class of c against targets around the loader's block"""
    rng = np.random.default_rng(2316)
    ns, Ls = [50, 100, 200, 400, 800, 1600], [1, 64, 129, 255, 256, 1000]
    assert [LR.rows_per_lane(n) for n in ns] == list(LR.ROWS) and all(2 * n > 64 * LR.rows_per_lane(n) for n in ns)
    query = np.zeros((len(ns), 1600), np.float32)
    for i, n in enumerate(ns):
        query[i, :n] = LR.signal_levels(rng, n).astype(np.float32) / np.float32(32.0)
    target = rng.integers(-128, 128, (len(Ls), 1008)).astype(np.int8)
    for g, L in enumerate(Ls):
        target[g, :L] = LR.signal_levels(rng, L, lowest=True)
    got = stage_arrays(codec(), query, ns, 32.0, target, Ls)
    assert_hits(got, LR.hits(query, ns, 32.0, target, Ls), "classes")


@pytest.mark.parametrize("index", [i for i, c in enumerate(CATALOGUE) if c.stride <= 65536], ids=[c.name for c in CATALOGUE if c.stride <= 65536])
def test_swapped_match_gives_the_same_hits(index):
    """every catalogue call a match call can express (targets of at most 65 536 levels), the same cells both ways.  The match rule clamps
    its query to +-127, so both routes get the call's targets with -128 raised to -127 (test_stage_entry_catalogue holds -128 to numpy)"""
    call = CATALOGUE[index]
    c = codec()
    query, valid, target, target_len = call.arrays()
    target = np.maximum(target, -127)
    got = stage_arrays(c, query, valid, call.quant, target, target_len)
    want = swapped_match(c, query, valid, call.quant, target, target_len)
    assert_hits(got, want, call.name)
    assert (got[:, :, 0] != 0xFFFFFFFF).any()


def test_python_method():
    c = codec()
    rng = np.random.default_rng(5)
    z = rng.normal(0, 1.2, (6, 256)).astype(np.float32)
    target = rng.integers(-60, 61, (2, 4096)).astype(np.int8)
    target[0, 3000:3100] = batch.quantize_levels(z[2, :100], 32.0)   # the whole query of read 2 stands in target 0
    lens = [4096, 777]
    valid = [256, 255, 100, 17, 0, 300]
    hits = c.locate(torch.from_numpy(z).to(c.device), i32(valid).to(c.device), torch.from_numpy(target).to(c.device), i32(lens).to(c.device))
    torch.cuda.synchronize()
    got = hits.cpu().numpy().view(np.uint32)
    assert tuple(got.shape) == (6, 2, 2)
    assert_hits(got, LR.hits(z, valid, 32.0, target, lens), "method")
    assert got[2][0].tolist()[0] == 0 and got[2][0].tolist()[1] <= 3100 and got[4].tolist() == [EMPTY] * 2


# ---- 2. the fused call ----------------------------------------------------------------------------------------------------------------------
def targets_for(want_q, valid, quant, rng, stride=1200):
    """targets for reads whose queries are want_q (bits): noise around the whole query of two of the reads (cost 0 there), a noise row, a
    full-range row, a short row, and refused lengths"""
    z = want_q.view(np.float32)
    target = rng.integers(90, 128, (7, stride)).astype(np.int8)
    lens = []
    full = [i for i, v in enumerate(valid) if v > 0]
    planted = {}
    for g, i in enumerate((full[0], full[-1])):
        k = LR.M.quantize(z[i, : valid[i]], quant)
        at = 37 + 211 * g
        if at + len(k) <= stride:
            target[g, at : at + len(k)] = k
            planted[(i, g)] = True
        lens.append(stride - 5 * g)
    target[2] = np.clip(np.repeat(rng.integers(-70, 71, stride // 6 + 1), 6)[:stride] + rng.integers(-6, 7, stride), -127, 127)
    target[3] = rng.integers(-128, 128, stride)
    target[4, :3] = (5, -128, 7)
    return target, lens + [700, stride, 3, 0, stride + 1], planted


def run_fused(fr, N, rng, **kw):
    """one fused call over fr, its targets built around the expected queries; the planted reads must cost nothing"""
    n = fr.n
    signed = kw.get("signed", True)
    sig = [x if signed else x.view(np.uint16) for x in fr.reads]
    bg, en = kw.get("begin") or [None] * n, kw.get("end") or [None] * n
    o = kw.get("offset") if kw.get("offset") is not None else np.zeros(n, np.float32)
    s = kw.get("scale") if kw.get("scale") is not None else np.ones(n, np.float32)
    norm = kw.get("norm")
    want_q, _, Tp = query_rows(sig, bg, en, N, list(zip(o, s)), norm[0] if norm else None, kw.get("stats", 0))
    valid = [min(t, N) for t in Tp]
    target, lens, planted = targets_for(want_q, valid, 32.0, rng)
    run = LocateRun(fr, target, lens, N, 32.0, **kw).check()
    assert planted
    for i, g in planted:
        assert int(run.want[i][g][0]) == 0, "the planted query costs nothing"
    return run


SIZES = [0, 1, 7, 9, 513, 2049, 4101]


def test_given_constants_and_signedness():
    c = codec()
    rng = np.random.default_rng(11)
    reads = [sine_signal(rng, T) for T in SIZES]
    fr = Frames(c, reads, c.options(True, 2, 1, 1), False, slack=6)
    o, s = np.full(fr.n, O, np.float32), np.full(fr.n, S, np.float32)
    run_fused(fr, 1024, rng, offset=o, scale=s)                       # T' < N, T' = 0, T' > N
    run_fused(fr, 512, rng, signed=False, offset=o, scale=s)


@pytest.mark.parametrize("stats", [0, 1], ids=["range", "read"])
def test_med_mad_and_ranges(stats):
    c = codec()
    rng = np.random.default_rng(29 + stats)
    reads, bg, en = [], [], []
    for T in (0, 9, 513, 2049, 4101):
        x = sine_signal(rng, T)
        for b, e in ((3, TO_END), (8, T - 3 if T > 3 else T), (2001, 2600), (TO_END, 0)):
            reads.append(x)
            bg.append(b)
            en.append(e)
    fr = Frames(c, reads, c.options(True, 2, 1, 1))
    run_fused(fr, 1024, rng, begin=bg, end=en, norm=NORMS["med_mad"], stats=stats)
    run_fused(fr, 2048, rng, begin=bg, offset=np.full(fr.n, O, np.float32), scale=np.full(fr.n, S, np.float32))   # (given constants, odd begins)


def test_a_failing_read_among_passing_ones():
    c = codec()
    rng = np.random.default_rng(91)
    fr = Frames(c, [sine_signal(rng, T) for T in (5000, 3000, 2500, 900, 700)], c.options(True, 2, 1, 1))
    src = fr.src.clone()
    size = fr.size.clone()
    size[1] = int(u32(fr.size)[1]) // 2   # the frame of read 1 cut off in its middle
    fr.size = size
    cap = u32(fr.dcap).tolist()
    cap[3] = 2 * 900 - 16                 # read 3's slot is 8 samples short
    fr.dcap = i32(cap).to(c.device)
    dst = torch.zeros(fr.dst_bytes + 64, dtype=torch.uint8, device=c.device)
    res16 = torch.full((fr.n,), -8, dtype=torch.int32, device=c.device)
    c.decompress(src, fr.off, fr.size, dst, fr.doff, fr.dcap, res16, fr.opts)
    torch.cuda.synchronize()
    un = u32(res16).tolist()
    assert [_lib.is_error(v) for v in un] == [False, True, False, True, False], [hex(v) for v in un]
    target = rng.integers(-60, 61, (3, 640)).astype(np.int8)
    for kw in ({"offset": [O] * 5, "scale": [S] * 5}, {"norm": (R.BONITO, batch.MED_MAD)}):
        run = LocateRun(fr, target, [640, 0, 333], 256, src=src, **kw).check(expect={1: un[1], 3: un[3]})
        got = run.a.out.cpu().numpy().view(np.uint32)
        assert got[1].tolist() == [EMPTY] * 3 and got[3].tolist() == [EMPTY] * 3
        assert got[0][0].tolist() != EMPTY and got[4][2].tolist() != EMPTY and got[2][1].tolist() == EMPTY


# ---- 3. POD5 ----------------------------------------------------------------------------------------------------------------------------------
POD5_SHAPES = [[1500], [13, 7, 1, 2047, 2049], [800, 0, 800], [24, 8, 2056, 16], [300] * 10, [], [0, 0], [2048, 100]]


def pod5_targets(sig, bg, en, N, consts, norm, stats, rng):
    want_q, _, Tp = query_rows(sig, bg, en, N, consts, norm, stats)
    return targets_for(want_q, [min(t, N) for t in Tp], 32.0, rng)[:2]


def test_pod5_reads_of_several_rows():
    c = codec()
    rows, first, frames = frames_of(71, POD5_SHAPES)
    n = len(first)
    rng = np.random.default_rng(3)
    o, s = np.full(n, O, np.float32), np.full(n, S, np.float32)
    consts = list(zip(o, s))
    sig = pod5_signals(rows, first)
    target, lens = pod5_targets(sig, [None] * n, [None] * n, 1024, consts, None, 0, rng)
    call = LocateCall(c, frames, rows, first, target, lens, 1024, offset=o, scale=s)
    assert call.call() == 0, c.L.vbz_gpu_last_error(c.ctx)
    expect_results(call, rows, first, 4)
    call.check(consts=consts)
    bg, en = [3, 8, 3, 2000, 701, TO_END, 0, 5], [TO_END, 3000, 1000, 2100, TO_END, 0, TO_END, 2100]
    for stats in (0, 1):
        target, lens = pod5_targets(sig, bg, en, 512, None, R.BONITO, stats, rng)
        call = LocateCall(c, frames, rows, first, target, lens, 512, begin=bg, end=en, norm=batch.MED_MAD, stats=stats)
        assert call.call(read_result=stats == 0) == 0, c.L.vbz_gpu_last_error(c.ctx)   # (stats 1: the caller takes no read_result)
        call.check(norm=R.BONITO)


def test_the_python_methods():
    c = codec()
    lens = [0, 1, 9, 513, 2049, 4101]
    rows, first, frames = frames_of(73, [[n] for n in lens])
    fr = Frames(c, rows, batch.pod5_options(), comp=arena(c, frames, 64))
    rng = np.random.default_rng(7)
    dev = c.device
    src, off, size = arena(c, frames, 16)
    want_q, _, Tp = query_rows(rows, [None] * 6, [None] * 6, 256, [(O, S)] * 6)
    valid = [min(t, 256) for t in Tp]
    target, tl, _ = targets_for(want_q, valid, 32.0, rng)
    t_d, len_d = torch.from_numpy(target).to(dev), i32(tl).to(dev)
    od, sd = torch.full((6,), O, dtype=torch.float32, device=dev), torch.full((6,), S, dtype=torch.float32, device=dev)
    res = torch.full((6,), -8, dtype=torch.int32, device=dev)
    hits, query = c.pod5_signal_locate(src, off, size, i32(lens).to(dev), list(range(6)), res, t_d, len_d, batch.Locate(256, 32.0), scale=sd, offset=od)
    res2 = torch.full((6,), -8, dtype=torch.int32, device=dev)
    hits2, query2 = c.signal_locate(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res2, fr.opts, t_d, len_d, batch.Locate(256, 32.0), scale=sd, offset=od)
    torch.cuda.synchronize()
    want = LR.hits(want_q.view(np.float32), valid, 32.0, target, tl)
    for h, q, r in ((hits, query, res), (hits2, query2, res2)):
        assert (q.cpu().numpy().view(np.uint32) == want_q).all()
        assert_hits(h.cpu().numpy().view(np.uint32), want, "method")
        assert u32(r).tolist() == [4 * t for t in lens]
