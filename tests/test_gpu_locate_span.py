"""Signal locate with the start of the stretch on the MI355X (include/vbz_gpu.h: the three *_locate_span_batch calls).  The stage entry runs
locate_ref's whole catalogue and the calls of locate_span_ref behind it -- plants at a target's very start and very end, tripled levels,
two equal plants, runs of the query's first level in front of a plant on each side of the loader's block of 256 steps, touching it or not
and reaching level 0, end - 1 at every residue of a dword, a walk back of more than 50 000 steps -- and two dense sweeps of every n
against every L up to 136, every {cost, end, start, 0} bit for bit against numpy and every (cost, end) against vbz_gpu_locate_batch.  The
same cells through vbz_gpu_match_span_batch with the roles swapped must give the same spans.  The fused calls are held to the statement
applied to the numpy-decoded signal; vbz_gpu_match_best_batch over a locate span arena, queued behind it, gives the winners' table."""
import numpy as np
import pytest
import torch

import locate_ref as LR
import locate_span_ref as LS
import match_path_ref as P
import norm_ref as R
from locate_span_support import EMPTY, SpanCall, SpanRun, stage, stage_arrays, swapped_match_span
from match_support import assert_hits, query_rows
from ranges_ref import pod5_signals
from test_gpu_locate import O, POD5_SHAPES, S, SIZES, TO_END, pod5_targets, targets_for
from typed_support import NORMS, Frames, arena, codec, expect_results, frames_of, i32, sine_signal, u32
from vbz_compression_amd import _lib, batch

pytestmark = pytest.mark.gpu

CATALOGUE = LS.catalogue()
SHORT = [i for i, c in enumerate(CATALOGUE) if c.stride <= 65536]


# ---- 1. the stage entry ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(CATALOGUE)), ids=[c.name for c in CATALOGUE])
def test_stage_entry_catalogue(index):
    call = CATALOGUE[index]
    c = codec()
    got = stage(c, call)
    for (read, tg), hit in call.planted.items():
        assert tuple(int(v) for v in got[read][tg][: len(hit)]) == hit, (call.name, "planted", read, tg, got[read][tg].tolist(), hit)
    assert_hits(got, LS.expected(index), call.name)
    for g in [g for g, L in enumerate(call.target_len) if L == 0 or L > call.stride]:
        assert (got[:, g] == np.array(EMPTY, np.uint32)).all(), (call.name, "refused column", g)
    for i in [i for i, v in enumerate(call.valid) if v == 0]:
        assert (got[i] == np.array(EMPTY, np.uint32)).all(), (call.name, "valid 0", i)
    ok = got[:, :, 0] != 0xFFFFFFFF
    assert (got[:, :, 2][ok] < got[:, :, 1][ok]).all() and (got[:, :, 3] == 0).all()
    assert_hits(got[:, :, :2], stage(c, call, cost_only=True), (call.name, "the cost-only call"))


@pytest.mark.parametrize("which", ["signal", "ties"])
def test_dense_sweep(which):
    """every n = 1 ... 136 against every L = 1 ... 136 in one call: signal-like levels with junk behind every read's and target's end, and
    levels of +-2, where many paths tie"""
    if which == "signal":
        query, valid, target, target_len, _ = LR.sweep()
        want = LS.sweep_expected()
    else:
        query, valid, target, target_len, want = LS.tie_sweep()
    assert query.shape == (136, 136) and target.shape == (136, 144) and want.shape == (136, 136, 4)
    c = codec()
    got = stage_arrays(c, query, valid, 32.0, target, target_len)
    assert_hits(got, want, which)
    assert_hits(got[:, :, :2], stage_arrays(c, query, valid, 32.0, target, target_len, cost_only=True), (which, "the cost-only call"))
    if which == "ties":   # the ties are there: most stretches are wider or narrower than the query
        assert ((got[:, :, 1] - got[:, :, 2]) != np.arange(1, 137)[:, None]).mean() > 0.5


def test_the_long_walk_back():
    """the answer known without the DP: more than 50 000 steps back, across the 65 536 line"""
    call = CATALOGUE[-1]
    assert call.name == "span-long" and call.stride == 70_016
    got = stage(codec(), call)
    assert got[0][0].tolist() == [0, LR.LONG_END, LS.LONG_START, 0] and LR.LONG_END - LS.LONG_START > 50_000 and LS.LONG_START < 65536 < LR.LONG_END


@pytest.mark.parametrize("index", SHORT, ids=[CATALOGUE[i].name for i in SHORT])
def test_swapped_match_span_gives_the_same_spans(index):
    """every call a match span call can express (targets of at most 65 536 levels), the same cells both ways; -128 raised to -127 on both
    sides, as test_gpu_locate does"""
    call = CATALOGUE[index]
    c = codec()
    query, valid, target, target_len = call.arrays()
    target = np.maximum(target, -127)
    got = stage_arrays(c, query, valid, call.quant, target, target_len)
    want = swapped_match_span(c, query, valid, call.quant, target, target_len)
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
    hits = c.locate_span(torch.from_numpy(z).to(c.device), i32(valid).to(c.device), torch.from_numpy(target).to(c.device), i32(lens).to(c.device))
    torch.cuda.synchronize()
    got = hits.cpu().numpy().view(np.uint32)
    assert tuple(got.shape) == (6, 2, 4)
    assert_hits(got, LS.spans(z, valid, 32.0, target, lens), "method")
    assert got[2][0].tolist()[0] == 0 and got[2][0].tolist()[1] <= 3100 and got[4].tolist() == [EMPTY] * 2


# ---- 2. the fused call ----------------------------------------------------------------------------------------------------------------------
def run_fused(fr, N, rng, **kw):
    """one fused call over fr, its targets built around the expected queries (test_gpu_locate.targets_for); the planted reads cost nothing"""
    n = fr.n
    signed = kw.get("signed", True)
    sig = [x if signed else x.view(np.uint16) for x in fr.reads]
    bg, en = kw.get("begin") or [None] * n, kw.get("end") or [None] * n
    o = kw.get("offset") if kw.get("offset") is not None else np.zeros(n, np.float32)
    s = kw.get("scale") if kw.get("scale") is not None else np.ones(n, np.float32)
    norm = kw.get("norm")
    want_q, _, Tp = query_rows(sig, bg, en, N, list(zip(o, s)), norm[0] if norm else None, kw.get("stats", 0))
    target, lens, planted = targets_for(want_q, [min(t, N) for t in Tp], 32.0, rng)
    run = SpanRun(fr, target, lens, N, 32.0, **kw).check()
    assert planted
    for i, g in planted:
        assert int(run.want[i][g][0]) == 0 and int(run.want[i][g][2]) < int(run.want[i][g][1]), "the planted query costs nothing"
    return run


def test_given_constants_and_signedness():
    c = codec()
    rng = np.random.default_rng(11)
    fr = Frames(c, [sine_signal(rng, T) for T in SIZES], c.options(True, 2, 1, 1), False, slack=6)
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
    run = SpanRun(fr, target, [640, 0, 333], 256, src=src, norm=(R.BONITO, batch.MED_MAD)).check(expect={1: un[1], 3: un[3]})
    got = run.a.out.cpu().numpy().view(np.uint32)
    assert got[1].tolist() == [EMPTY] * 3 and got[3].tolist() == [EMPTY] * 3
    assert got[0][0].tolist() != EMPTY and got[4][2].tolist() != EMPTY and got[2][1].tolist() == EMPTY


# ---- 3. POD5 ----------------------------------------------------------------------------------------------------------------------------------
def test_pod5_reads_of_several_rows():
    c = codec()
    rows, first, frames = frames_of(71, POD5_SHAPES)
    n = len(first)
    rng = np.random.default_rng(3)
    o, s = np.full(n, O, np.float32), np.full(n, S, np.float32)
    consts = list(zip(o, s))
    sig = pod5_signals(rows, first)
    target, lens = pod5_targets(sig, [None] * n, [None] * n, 1024, consts, None, 0, rng)
    call = SpanCall(c, frames, rows, first, target, lens, 1024, offset=o, scale=s)
    assert call.call() == 0, c.L.vbz_gpu_last_error(c.ctx)
    expect_results(call, rows, first, 4)
    call.check(consts=consts)
    bg, en = [3, 8, 3, 2000, 701, TO_END, 0, 5], [TO_END, 3000, 1000, 2100, TO_END, 0, TO_END, 2100]
    target, lens = pod5_targets(sig, bg, en, 512, None, R.BONITO, 1, rng)
    call = SpanCall(c, frames, rows, first, target, lens, 512, begin=bg, end=en, norm=batch.MED_MAD, stats=1)
    assert call.call(read_result=False) == 0, c.L.vbz_gpu_last_error(c.ctx)   # (the caller takes no read_result)
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
    hits, query = c.pod5_signal_locate_span(src, off, size, i32(lens).to(dev), list(range(6)), res, t_d, len_d, batch.Locate(256, 32.0), scale=sd, offset=od)
    res2 = torch.full((6,), -8, dtype=torch.int32, device=dev)
    hits2, query2 = c.signal_locate_span(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res2, fr.opts, t_d, len_d, batch.Locate(256, 32.0), scale=sd, offset=od)
    torch.cuda.synchronize()
    want = LS.spans(want_q.view(np.float32), valid, 32.0, target, tl)
    for h, q, r in ((hits, query, res), (hits2, query2, res2)):
        assert tuple(h.shape) == (6, len(tl), 4)
        assert (q.cpu().numpy().view(np.uint32) == want_q).all()
        assert_hits(h.cpu().numpy().view(np.uint32), want, "method")
        assert u32(r).tolist() == [4 * t for t in lens]


# ---- 4. the winners' table ------------------------------------------------------------------------------------------------------------------
def test_span_then_best_with_no_host_copy():
    """vbz_gpu_match_best_batch queued behind the span call on the same arena: each read's best target and its [begin, end) in target
    coordinates.  A max_cost excludes some reads; one read has every target refused for it (valid 0)"""
    c = codec()
    rng = np.random.default_rng(4235)
    N, stride, Gn = 128, 4096, 5
    target = rng.integers(-60, 61, (Gn, stride)).astype(np.int8)
    lens = [4096, 3000, 0, 4097, 2500]
    levels = [LR.distinct_levels(rng, n) for n in (100, 128, 77, 128, 50, 128)]
    target[0, 3500 : 3500 + 100] = levels[0]                       # read 0 stands in target 0, far from its start ...
    target[4, 40 : 40 + 3 * 77] = np.repeat(levels[2], 3)          # ... read 2 tripled in target 4
    target[1, 2000 : 2000 + 128] = levels[3]
    target[4, 1000 : 1000 + 128] = levels[3]                       # read 3 in two targets: the smaller index wins
    query = np.zeros((6, N), np.float32)
    for i, k in enumerate(levels):
        query[i, : len(k)] = k.astype(np.float32) / np.float32(32.0)
    valid = [100, 128, 77, 128, 0, 128]
    got, out = stage_arrays(c, query, valid, 32.0, target, lens, keep_out=True)
    want = LS.spans(query, valid, 32.0, target, lens)
    assert_hits(got, want, "spans")
    max_cost = 300
    pairs = torch.full((7, 4), 0x5A5A5A5A, dtype=torch.int32, device=c.device)
    rc = c.L.vbz_gpu_match_best_batch(c.ctx, 6, out.data_ptr(), Gn, max_cost, pairs.data_ptr())
    c.synchronize()
    assert rc == 0, c.L.vbz_gpu_last_error(c.ctx)
    table = pairs.cpu().numpy().view(np.uint32)
    assert (table[6] == 0x5A5A5A5A).all()
    assert (table[:6] == P.best(want, max_cost)).all(), (table[:6].tolist(), P.best(want, max_cost).tolist())
    assert table[0].tolist() == [0, 0, 3500, 3600] and table[2].tolist() == [2, 4, 40, 40 + 3 * 77 - 2] and table[3].tolist() == [3, 1, 2000, 2128]
    assert table[4].tolist() == [4, 0xFFFFFFFF, 0, 0]                                        # every target refused
    excluded = [i for i in (1, 5) if want[i, :, 0].min() > max_cost]
    assert excluded and all(table[i].tolist() == [i, 0xFFFFFFFF, 0, 0] for i in excluded)   # ... and the reads max_cost excludes
    by_method = c.match_best(out[:6], max_cost).cpu().numpy().view(np.uint32)
    assert (by_method == table[:6]).all()
