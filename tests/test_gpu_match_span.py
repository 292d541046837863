"""Signal match with the start of the aligned stretch on the MI355X (include/vbz_gpu.h: vbz_gpu_match_span and the three
*_match_span_batch calls).  The stage entry runs match_ref's catalogue and match_span_ref's -- ties over small alphabets, planted
starts, the extremes of the packed key's fields, and one data set on both sides of the host's choice between the packed and the wide
kernel -- every entry bit for bit against match_span_ref.spans, `zero` 0, (cost, end) equal to what vbz_gpu_match_batch writes for the
same inputs, canaries behind every arena.  The fused calls are held to the statement applied to the numpy-decoded signal over short
reads: both codec versions and POD5 rows, given constants and MED_MAD, odd range begins, an empty range, a failing read."""
import numpy as np
import pytest
import torch

import match_ref as M
import match_span_ref as S
import norm_ref as R
from match_support import assert_hits, query_rows
from match_span_support import EMPTY, SpanCall, SpanRun, stage_span
from ranges_ref import pod5_signals
from typed_support import NORMS, Frames, arena, codec, frames_of, i32, sine_signal, u32
from vbz_compression_amd import _lib, batch

pytestmark = pytest.mark.gpu

TO_END = 0xFFFFFFFF
O, SC = -330.0, 1.0 / 45.0   # given constants that bring sine_signal to about unit scale
CALLS = [(True, i, c.name) for i, c in enumerate(M.catalogue())] + [(False, i, c.name) for i, c in enumerate(S.span_catalogue())]


# ---- 1. the stage entry over both catalogues --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base,index", [(b, i) for b, i, _ in CALLS], ids=[("match-" if b else "") + name for b, _, name in CALLS])
def test_stage_entry_catalogue(base, index):
    call = (M.catalogue() if base else S.span_catalogue())[index]
    c = codec()
    got = stage_span(c, call)
    want = S.expected(index, base)
    for (read, ref), hit in call.planted.items():   # (match_ref plants (cost, end), match_span_ref (cost, end, start))
        assert tuple(int(v) for v in got[read][ref][: len(hit)]) == hit, (call.name, "planted", read, ref, got[read][ref].tolist(), hit)
    assert_hits(got, want, call.name)
    assert (got[:, :, 3] == 0).all(), "zero"
    for r in [r for r, m in enumerate(call.ref_len) if m == 0 or m > call.stride]:
        assert (got[:, r] == np.array(EMPTY, np.uint32)).all(), (call.name, "refused column", r)
    # (cost, end) are the cost-only call's, launch against launch
    assert_hits(got[:, :, :2], stage_span(c, call, cost_only=True), (call.name, "against vbz_gpu_match_batch"))


def test_both_sides_of_the_hosts_rule_give_identical_hits():
    c = codec()
    rule = [call for call in S.span_catalogue() if call.name.startswith("rule")]
    assert [(call.N, call.stride) for call in rule] == [(4096, 2048), (8192, 2048), (16384, 416), (32768, 416)]
    got = [stage_span(c, call) for call in rule]
    for g, call in zip(got[1:], rule[1:]):
        assert_hits(g, got[0], call.name)
    assert (got[0][:, :, 0] != 0xFFFFFFFF).all()


def test_python_method():
    c = codec()
    rng = np.random.default_rng(5)
    z = rng.normal(0, 1.2, (7, 256)).astype(np.float32)
    ref = np.zeros((3, 64), np.int8)
    ref[0, :40] = batch.quantize_levels(z[2, 100:140], 32.0)   # a stretch of read 2 itself
    ref[1, :64] = rng.integers(-60, 61, 64)
    ref[2, :9] = rng.integers(-128, 128, 9)
    lens = [40, 64, 9]
    valid = [256, 255, 256, 17, 0, 300, 64]
    hits = c.match_span(torch.from_numpy(z).to(c.device), i32(valid).to(c.device), torch.from_numpy(ref).to(c.device), i32(lens).to(c.device))
    torch.cuda.synchronize()
    got = hits.cpu().numpy().view(np.uint32)
    assert tuple(got.shape) == (7, 3, 4)
    assert_hits(got, S.spans(z, valid, 32.0, ref, lens), "method")
    assert got[2][0].tolist()[0] == 0 and got[2][0].tolist()[1] - got[2][0].tolist()[2] <= 80 and got[4].tolist() == [EMPTY] * 3


# ---- 2. the fused call ----------------------------------------------------------------------------------------------------------------------
SIZES = [0, 1, 7, 9, 63, 64, 65, 129, 300, 513, 700, 1000, 1500, 2049, 2500, 3000]
BEGIN = [3, 3, 3, 8, 3, 1, 3, 3, 3, TO_END, 3, 701, 3, 3, 8, 5]   # (read 9: the empty range)
END = [TO_END] * 9 + [0] + [TO_END, 1000, TO_END, 2100, TO_END, TO_END]


def refs_from(want_q, valid, quant, rng, skip=(), stride=416):
    """references for reads whose queries are want_q (bits): stretches of two of the queries themselves (cost 0 there), plateaus of M = 400,
    a small alphabet of M = 33, and refused lengths"""
    z = want_q.view(np.float32)
    long = [i for i, v in enumerate(valid) if v >= min(z.shape[1], 320) and i not in skip]
    ref = np.zeros((6, stride), np.int8)
    lens = []
    for r, i in enumerate((long[0], long[-1])):
        at = 37 + 64 * r
        k = M.quantize(z[i, at : at + 150 + 61 * r], quant)
        ref[r, : len(k)] = k
        lens.append(len(k))
    ref[2, :400] = np.clip(np.repeat(rng.integers(-70, 71, 67), 6)[:400] + rng.integers(-6, 7, 400), -127, 127)
    ref[3, :33] = rng.integers(-3, 4, 33)
    ref[4, :20] = 5
    ref[5, :20] = 5
    return ref, lens + [400, 33, 0, stride + 1], (long[0], long[-1])


@pytest.mark.parametrize("norm", [None, "med_mad"])
@pytest.mark.parametrize("version", [0, 1])
def test_fused_call_over_short_reads(version, norm):
    c = codec()
    rng = np.random.default_rng(17 + version)
    reads = [sine_signal(rng, T) for T in SIZES]
    fr = Frames(c, reads, c.options(True, 2, 1, version))
    # read 12 fails: its frame is cut off in its middle.  Its verdict is whatever the plain decode says
    size = fr.size.clone()
    size[12] = int(u32(fr.size)[12]) // 2
    fr.size = size
    dst = torch.zeros(fr.dst_bytes + 64, dtype=torch.uint8, device=c.device)
    res16 = torch.full((fr.n,), -8, dtype=torch.int32, device=c.device)
    c.decompress(fr.src, fr.off, fr.size, dst, fr.doff, fr.dcap, res16, fr.opts)
    torch.cuda.synchronize()
    un = u32(res16).tolist()
    assert [i for i, v in enumerate(un) if _lib.is_error(v)] == [12], [hex(v) for v in un]
    kw = {"norm": NORMS[norm]} if norm else {"offset": np.full(fr.n, O, np.float32), "scale": np.full(fr.n, SC, np.float32)}
    consts = list(zip(kw.get("offset", np.zeros(fr.n)), kw.get("scale", np.ones(fr.n))))
    want_q, _, Tp = query_rows(fr.reads, BEGIN, END, 512, consts, NORMS[norm][0] if norm else None, 0)
    ref, lens, planted = refs_from(want_q, [min(t, 512) for t in Tp], 32.0, rng, skip=(12,))
    run = SpanRun(fr, ref, lens, 512, 32.0, begin=BEGIN, end=END, **kw).check(expect={12: un[12]})
    got = run.a.out.cpu().numpy().view(np.uint32)
    assert got[12].tolist() == [EMPTY] * 6 and got[9].tolist() == [EMPTY] * 6 and got[0].tolist() == [EMPTY] * 6
    for r, i in enumerate(planted):
        assert int(got[i][r][0]) == 0 and int(got[i][r][2]) < int(got[i][r][1]), (i, r, got[i][r].tolist())
    assert (got[: fr.n, 4:] == np.array(EMPTY, np.uint32)).all()


# ---- 3. POD5 ----------------------------------------------------------------------------------------------------------------------------------
POD5_SHAPES = [[1500], [13, 7, 1, 2047, 2049], [800, 0, 800], [24, 8, 2056, 16], [300] * 8, [], [0, 0], [2048, 100]]
POD5_BEGIN = [3, 8, 3, 2001, 701, TO_END, 0, 5]
POD5_END = [TO_END, 3000, 1001, 2100, TO_END, 0, TO_END, 2100]


@pytest.mark.parametrize("norm", [None, "med_mad"])
def test_pod5_reads(norm):
    c = codec()
    rows, first, frames = frames_of(74, POD5_SHAPES)
    n = len(first)
    rng = np.random.default_rng(3)
    o, s = np.full(n, O, np.float32), np.full(n, SC, np.float32)
    consts = None if norm else list(zip(o, s))
    sig = pod5_signals(rows, first)
    want_q, _, Tp = query_rows(sig, POD5_BEGIN, POD5_END, 512, consts, R.BONITO if norm else None, 0)
    damaged = list(frames)
    damaged[first[2]] = frames[first[2]][: len(frames[first[2]]) // 2]   # read 2's first row is cut off: the read fails
    ref, lens, planted = refs_from(want_q, [min(t, 512) for t in Tp], 32.0, rng, skip=(2,))
    kw = {"norm": batch.MED_MAD} if norm else {"offset": o, "scale": s}
    call = SpanCall(c, damaged, rows, first, ref, lens, 512, begin=POD5_BEGIN, end=POD5_END, **kw)
    assert call.call() == 0, c.L.vbz_gpu_last_error(c.ctx)
    assert _lib.is_error(u32(call.read_result)[2]) and not any(_lib.is_error(v) for i, v in enumerate(u32(call.read_result)[:n]) if i != 2)
    call.check(norm=R.BONITO if norm else None, consts=consts, failed={2})
    got = call.a.out.cpu().numpy().view(np.uint32)
    assert got[2].tolist() == [EMPTY] * 6 and got[5].tolist() == [EMPTY] * 6
    for r, i in enumerate(planted):
        assert int(got[i][r][0]) == 0 and int(got[i][r][2]) < int(got[i][r][1]), (i, r, got[i][r].tolist())


def test_the_python_methods_of_the_fused_calls():
    c = codec()
    lens = [0, 1, 9, 513, 2049, 4101]
    rows, first, frames = frames_of(73, [[n] for n in lens])
    fr = Frames(c, rows, batch.pod5_options(), comp=arena(c, frames, 64))
    rng = np.random.default_rng(7)
    dev = c.device
    src, off, size = arena(c, frames, 16)
    want_q, _, Tp = query_rows(rows, [None] * 6, [None] * 6, 256, [(O, SC)] * 6)
    valid = [min(t, 256) for t in Tp]
    ref, rl, _ = refs_from(want_q, valid, 32.0, rng)
    ref_d, len_d = torch.from_numpy(ref).to(dev), i32(rl).to(dev)
    od, sd = torch.full((6,), O, dtype=torch.float32, device=dev), torch.full((6,), SC, dtype=torch.float32, device=dev)
    res = torch.full((6,), -8, dtype=torch.int32, device=dev)
    hits, query = c.pod5_signal_match_span(src, off, size, i32(lens).to(dev), list(range(6)), res, ref_d, len_d, batch.Match(256, 32.0), scale=sd, offset=od)
    res2 = torch.full((6,), -8, dtype=torch.int32, device=dev)
    hits2, query2 = c.signal_match_span(fr.src, fr.off, fr.size, fr.doff, fr.dcap, res2, fr.opts, ref_d, len_d, batch.Match(256, 32.0), scale=sd, offset=od)
    torch.cuda.synchronize()
    want = S.spans(want_q.view(np.float32), valid, 32.0, ref, rl)
    for h, q, r in ((hits, query, res), (hits2, query2, res2)):
        assert tuple(h.shape) == (6, 6, 4)
        assert (q.cpu().numpy().view(np.uint32) == want_q).all()
        assert_hits(h.cpu().numpy().view(np.uint32), want, "method")
        assert u32(r).tolist() == [4 * t for t in lens]
