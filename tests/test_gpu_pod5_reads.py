"""POD5 reads of several rows on the MI355X (include/vbz_gpu.h: vbz_gpu_pod5_reads): the chunk store and the statistics see a read's rows
as one signal.  Chunks, shift / scale and the normalised typed signal are held bit for bit to tests/pod5_reads_ref.py (the chunking rules
and norm_ref on the concatenated rows) for grouping shapes that reach every boundary of the svb16 tile (2 048 samples) and of a 16-byte
line, on the one-wavefront and the large-read path, in split and routed call shapes; then verdicts, untrusted tables, refusals."""
import ctypes

import numpy as np
import pytest
import torch

import norm_ref as R
import oracle_lib as O
import pod5_ref as P
import pod5_reads_ref as PR
from typed_support import CANARY, ELEM, SHAPES, TORCH, Call, arena, check_chunks, codec, expect_results, frames_of, i32, pod5_compress, u32
from vbz_compression_amd import _lib, batch

pytestmark = pytest.mark.gpu

E_ZSTD, E_INPUT, E_DEST, E_STREAM = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFC, 0xFFFFFFFB

CHUNKINGS = [(8, 8, "pad", 0), (1024, 1000, "pad", 0), (4096, 4096, "pad", 0), (1024, 1000, "end", 1), (1024, 1000, "end", 6), (1024, 1000, "end", 8),
             (8, 8, "end", 6)]


# ---- grouping shapes, chunk parameters, dtypes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("segmented", [0, 1])
@pytest.mark.parametrize("chunking", CHUNKINGS, ids=lambda c: "L%d-S%d-%s%d" % c)
def test_grouping_shapes_chunks(segmented, chunking):
    c = codec(VBZ_HIP_SEGMENTED=segmented)
    rows, first, frames = frames_of(1, SHAPES)
    rng = np.random.default_rng(3)
    o = rng.uniform(-600, 600, len(first)).astype(np.float32)
    s = rng.uniform(0.01, 2.5, len(first)).astype(np.float32)
    for dtype in (("f32", "f16", "bf16") if chunking[0] == 1024 and chunking[2] == "end" and chunking[3] == 6 else ("f16",)):
        call = Call(c, frames, [len(x) for x in rows], PR.bounds(first, len(rows)), dtype, chunking, offset=o, scale=s)
        assert call.chunk_call() == 0, c.L.vbz_gpu_last_error(c.ctx)
        expect_results(call, rows, first, ELEM[dtype])
        check_chunks(call, rows, first, chunking, list(zip(o, s)))


def test_one_row_read_equals_row_wise_call_and_chunk_info():
    c = codec()
    rows, first, frames = frames_of(1, SHAPES)
    src, off, size = arena(c, frames, 16)
    samples = i32([len(x) for x in rows]).to(c.device)
    res = torch.full((len(rows),), -8, dtype=torch.int32, device=c.device)
    ch, cf, info, rr = c.pod5_decompress_chunks(src, off, size, samples, first, res, 1024, 1000, mode="end", end_align=6, pad=-7.0)
    res1 = torch.full((1,), -8, dtype=torch.int32, device=c.device)
    ch1, cf1, _ = c.decompress_chunks(src, off[:1].contiguous(), size[:1].contiguous(), samples[:1].contiguous(), res1, batch.pod5_options(), 1024, 1000,
                                      mode="end", end_align=6, pad=-7.0)
    torch.cuda.synchronize()
    cf = cf.cpu().numpy()
    assert torch.equal(ch[cf[0] : cf[1]].view(torch.int16), ch1.view(torch.int16))
    sig = PR.read_signals(rows, first)
    want = [(k, a) for k, x in enumerate(sig) for a in PR.chunk_starts(len(x), 1024, 1000, "end", 6)]
    assert info.cpu().numpy().tolist() == [list(w) for w in want]
    assert u32(rr).tolist() == [2 * len(x) for x in sig]


# ---- statistics ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("segmented", [0, 1])
@pytest.mark.parametrize("signed", [True, False])
def test_statistics_alone_small_shapes(segmented, signed):
    c = codec(VBZ_HIP_SEGMENTED=segmented)
    rows, first, frames = frames_of(1, SHAPES)
    sig = PR.read_signals(rows, first)
    for p, nm in ((R.BONITO, batch.MED_MAD), (R.DORADO, batch.DORADO_QUANTILE)):
        call = Call(c, frames, [len(x) for x in rows], PR.bounds(first, len(rows)), norm=nm)
        assert call.stats_call(signed) == 0
        expect_results(call, rows, first, 2)
        ss = call.ss.cpu().numpy()
        for k, x in enumerate(sig):
            shift, scale, _, _ = PR.shift_scale(x, p, signed)
            assert (ss[k][0].view(np.uint32), ss[k][1].view(np.uint32)) == (shift.view(np.uint32), scale.view(np.uint32)), (p[0], k, len(x))


def test_normalised_chunks_small_shapes():
    c = codec()
    rows, first, frames = frames_of(1, SHAPES)
    sig = PR.read_signals(rows, first)
    chunking = (1024, 1000, "end", 6)
    for p, nm in ((R.BONITO, batch.MED_MAD), (R.DORADO, batch.DORADO_QUANTILE)):
        call = Call(c, frames, [len(x) for x in rows], PR.bounds(first, len(rows)), "f16", chunking, norm=nm)
        assert call.chunk_call() == 0
        expect_results(call, rows, first, 2)
        check_chunks(call, rows, first, chunking, [PR.shift_scale(x, p)[2:] for x in sig])


# ---- real signal ------------------------------------------------------------------------------------------------------------------
_golden = None


def golden():
    """(rows, first_row, reads, libzstd frames, library frames) of the golden reads cut into rows of 102 400 samples"""
    global _golden
    if _golden is None:
        rows, owner = P.golden_rows()
        first = [i for i in range(len(rows)) if i == 0 or owner[i] != owner[i - 1]]
        own = pod5_compress(codec(), rows)
        _golden = (rows, first, PR.read_signals(rows, first), [P.compress_row(x) for x in rows], own)
    return _golden


@pytest.mark.parametrize("writer", ["libzstd", "library"])
def test_real_signal_normalised_chunks_and_signal(writer):
    c = codec()
    rows, first, sig, ref_frames, own_frames = golden()
    frames = ref_frames if writer == "libzstd" else own_frames
    samples = [len(x) for x in rows]
    table = PR.bounds(first, len(rows))
    for mode, ea in (("pad", 0), ("end", 8)):
        chunking = (4000, 3600, mode, ea)
        for p, nm, signed in ((R.BONITO, batch.MED_MAD, True), (R.DORADO, batch.DORADO_QUANTILE, True), (R.DORADO, batch.DORADO_QUANTILE, False)):
            if signed is False and mode == "end":
                continue
            call = Call(c, frames, samples, table, "f16", chunking, norm=nm, signed=signed)
            assert call.chunk_call() == 0
            expect_results(call, rows, first, 2)
            ss = call.ss.cpu().numpy()
            consts = []
            for k, x in enumerate(sig):
                shift, scale, so, sc = PR.shift_scale(x, p, signed)
                assert (ss[k][0].view(np.uint32), ss[k][1].view(np.uint32)) == (shift.view(np.uint32), scale.view(np.uint32)), (p[0], signed, k)
                consts.append((so, sc))
            if signed:   # (the reference's typed_bits takes int16 values: the uint16 reading is held to its statistics)
                check_chunks(call, rows, first, chunking, consts)
    # the normalised typed signal over pod5_read_layout: every read contiguous, normalised by its own statistics
    src, off, size = arena(c, frames, 16)
    for dtype in ("f32", "f16"):
        res = torch.full((len(rows),), -8, dtype=torch.int32, device=c.device)
        out, lay, rr = c.pod5_decompress_signal_norm(src, off, size, samples, first, res, batch.MED_MAD, dtype=TORCH[dtype])
        torch.cuda.synchronize()
        E = ELEM[dtype]
        assert u32(res).tolist() == [E * n for n in samples] and u32(rr).tolist() == [E * len(x) for x in sig]
        host = out.view(torch.uint8).cpu().numpy()
        for k, x in enumerate(sig):
            _, _, so, sc = PR.shift_scale(x, R.BONITO)
            want = PR.typed_bits(x, so, sc, dtype)
            o = int(lay.read_off[k])
            assert host[o : o + E * len(x)].view(want.dtype).tobytes() == want.tobytes(), (dtype, k)


# ---- call shapes ------------------------------------------------------------------------------------------------------------------
def test_split_halves_and_routed_row():
    rng = np.random.default_rng(11)
    shapes = [[int(v) for v in rng.integers(0, 900, int(rng.integers(1, 6)))] for _ in range(70)]
    n_rows = sum(len(s) for s in shapes)
    # a read whose rows straddle row n / 2
    acc, straddles = 0, False
    for s in shapes:
        straddles = straddles or (acc < n_rows // 2 < acc + len(s))
        acc += len(s)
    if not straddles:
        shapes[35] = shapes[35] + [40, 50, 60, 70, 80, 90, 100, 110]
    shapes.append([500, 300000, 700])   # a row of 600 KB: the int16 call would route it to the large-read path
    rows, first, frames = frames_of(11, shapes)
    half = len(rows) // 2
    b = PR.bounds(first, len(rows))
    assert any(b[k] < half < b[k + 1] for k in range(len(first)))
    chunking = (1024, 1000, "end", 6)
    outs = []
    for c in (codec(VBZ_HIP_SPLIT_MIN=64), codec(VBZ_HIP_SPLIT_MIN=0)):
        call = Call(c, frames, [len(x) for x in rows], b, "f16", chunking, norm=batch.MED_MAD)
        assert call.chunk_call() == 0
        expect_results(call, rows, first, 2)
        outs.append((call.chunks.cpu().numpy(), call.ss.cpu().numpy().tobytes(), call))
    assert (outs[0][0] == outs[1][0]).all() and outs[0][1] == outs[1][1]
    sig = PR.read_signals(rows, first)
    check_chunks(outs[0][2], rows, first, chunking, [PR.shift_scale(x, R.BONITO)[2:] for x in sig])


# ---- verdicts ---------------------------------------------------------------------------------------------------------------------
def test_failing_row_inside_a_read():
    c = codec()
    shapes = [[600, 700], [900, 1000, 1100], [500], [900, 1000, 1100], [640]]
    rows, first, good = frames_of(21, shapes)
    frames = list(good)
    frames[3] = good[3][: len(good[3]) // 2]                       # a damaged frame in the middle row of read 1
    frames[7] = O.zstd_compress(P.svb16_encode(rows[7])[:-1], 1)   # a stream with a byte cut off in the middle row of read 3
    samples = [len(x) for x in rows]
    # what the row-wise call says
    src, off, size = arena(c, frames, 16)
    res = torch.full((len(rows),), -8, dtype=torch.int32, device=c.device)
    c.decompress_chunks(src, off, size, i32(samples).to(c.device), res, batch.pod5_options(), 1024, 1000)
    torch.cuda.synchronize()
    row_wise = u32(res).tolist()
    assert row_wise[3] == E_ZSTD and row_wise[7] == E_STREAM
    chunking = (1024, 1000, "pad", 0)
    call = Call(c, frames, samples, PR.bounds(first, len(rows)), "f16", chunking, norm=batch.MED_MAD)
    assert call.chunk_call() == 0
    assert u32(call.result).tolist() == row_wise
    sig = PR.read_signals(rows, first)
    assert u32(call.read_result).tolist() == [2 * len(sig[0]), E_ZSTD, 2 * len(sig[2]), E_STREAM, 2 * len(sig[4])]
    check_chunks(call, rows, first, chunking, [PR.shift_scale(x, R.BONITO)[2:] for x in sig], skip=(1, 3))


def test_wrong_chunk_first_pair_fails_the_whole_read():
    c = codec()
    shapes = [[600, 700], [900, 1000, 1100], [500, 20]]
    rows, first, frames = frames_of(22, shapes)
    chunking = (1024, 1000, "pad", 0)
    sig = PR.read_signals(rows, first)
    counts = [len(PR.chunk_starts(len(x), 1024, 1000, "pad", 0)) for x in sig]   # 2, 3, 1
    cf = [0, counts[0], counts[0] + counts[1] + 1, counts[0] + counts[1] + 1 + counts[2]]   # read 1 claims one row too many
    call = Call(c, frames, [len(x) for x in rows], PR.bounds(first, len(rows)), "f16", chunking, chunk_first=cf)
    assert call.chunk_call() == 0
    assert u32(call.result).tolist() == [1200, 1400, E_DEST, E_DEST, E_DEST, 1000, 40]
    assert u32(call.read_result).tolist() == [2600, E_DEST, 1040]
    got = call.chunks.cpu().numpy().reshape(-1, 1024 * 2)
    assert (got[cf[1] : cf[2]] == CANARY).all(), "a read that failed the chunk check was written"
    check_chunks(call, rows, first, chunking, [(0.0, 1.0)] * 3, skip=(1,))


@pytest.mark.parametrize("table", [[1, 2, 5, 7], [0, 5, 2, 7], [0, 2, 5, 6], [0, 2, 5, 8]], ids=["first-1", "decreasing", "last-short", "last-long"])
def test_bad_first_row_fails_whole(table):
    c = codec()
    rows, first, frames = frames_of(22, [[600, 700], [900, 1000, 1100], [500, 20]])
    chunking = (1024, 1000, "pad", 0)
    call = Call(c, frames, [len(x) for x in rows], table, "f16", chunking, norm=batch.MED_MAD, chunk_first=[0, 2, 5, 6])
    assert call.chunk_call() == 0
    assert u32(call.result).tolist() == [E_INPUT] * 7 and u32(call.read_result).tolist() == [E_INPUT] * 3
    assert (call.chunks.cpu().numpy() == CANARY).all() and (call.ss.cpu().numpy() == -777.0).all()
    call = Call(c, frames, [len(x) for x in rows], table, norm=batch.MED_MAD)
    assert call.stats_call() == 0
    assert u32(call.result).tolist() == [E_INPUT] * 7 and u32(call.read_result).tolist() == [E_INPUT] * 3
    assert (call.ss.cpu().numpy() == -777.0).all()
    rs = torch.full((3,), -8, dtype=torch.int32, device=c.device)
    assert c.L.vbz_gpu_pod5_read_samples_batch(c.ctx, 7, i32([len(x) for x in rows]).to(c.device).data_ptr(), ctypes.byref(call.reads), rs.data_ptr()) == 0
    c.synchronize()
    assert u32(rs).tolist() == [E_INPUT] * 3


def test_read_samples():
    c = codec()
    samples = i32([5, 0, 7, 1 << 30, 1 << 30, 9]).to(c.device)
    table = i32([0, 3, 3, 5, 6]).to(c.device)
    r = _lib.GpuPod5Reads()
    r.n_reads, r.first_row = 4, table.data_ptr()
    out = torch.full((4,), -8, dtype=torch.int32, device=c.device)
    assert c.L.vbz_gpu_pod5_read_samples_batch(c.ctx, 6, samples.data_ptr(), ctypes.byref(r), out.data_ptr()) == 0
    c.synchronize()
    assert u32(out).tolist() == [12, 0, E_DEST, 9]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_host_refusals_launch_nothing():
    c = codec()
    rows, first, frames = frames_of(22, [[600, 700], [900, 1000, 1100], [500, 20]])
    samples, table, chunking = [len(x) for x in rows], PR.bounds(first, len(rows)), (1024, 1000, "pad", 0)

    def fresh(**kw):
        return Call(c, frames, samples, table, "f16", chunking, **kw)

    def untouched(call):
        assert (call.chunks.cpu().numpy() == CANARY).all() and (u32(call.result) == 0xFFFFFFF8).all() and (call.ss.cpu().numpy() == -777.0).all()

    call = fresh()
    call.opts = batch.GpuCodec.options(True, 2, 1, 0)          # not POD5 options
    assert call.chunk_call() == -2
    untouched(call)
    call = fresh()
    call.reads.reserved = 1
    assert call.chunk_call() == -2
    untouched(call)
    call = fresh()
    call.reads.first_row = None
    assert call.chunk_call() == -2
    untouched(call)
    call = fresh(norm=batch.MED_MAD, offset=np.zeros(3, np.float32))   # norm with given constants
    assert call.chunk_call() == -2
    untouched(call)
    call = fresh()
    call.ch.step = 12                                           # what the row-wise chunk call refuses
    assert call.chunk_call() == -2
    untouched(call)
    call = fresh()
    L = c.L
    assert L.vbz_gpu_pod5_decompress_chunks_batch(c.ctx, ctypes.byref(call.b), ctypes.byref(call.opts), ctypes.byref(call.f), ctypes.byref(call.ch), None,
                                                  call.chunk_first.data_ptr(), call.chunks.data_ptr(), call.rows, None, None) == -2   # NULL reads
    assert L.vbz_gpu_pod5_decompress_chunks_batch(c.ctx, ctypes.byref(call.b), ctypes.byref(call.opts), ctypes.byref(call.f), ctypes.byref(call.ch),
                                                  ctypes.byref(call.reads), None, call.chunks.data_ptr(), call.rows, None, None) == -2   # NULL chunk_first
    call.m = batch.MED_MAD.c_struct()
    assert L.vbz_gpu_pod5_signal_norm_batch(c.ctx, ctypes.byref(call.b), ctypes.byref(call.opts), 1, ctypes.byref(call.reads), ctypes.byref(call.m),
                                            None) == -2                                                                             # NULL shift_scale
    assert L.vbz_gpu_pod5_signal_norm_batch(c.ctx, ctypes.byref(call.b), ctypes.byref(call.opts), 1, None, ctypes.byref(call.m), call.ss.data_ptr()) == -2
    assert L.vbz_gpu_pod5_decompress_signal_norm_batch(c.ctx, ctypes.byref(call.b), ctypes.byref(call.opts), ctypes.byref(call.f), None,
                                                       ctypes.byref(call.m), None) == -2
    assert L.vbz_gpu_pod5_read_samples_batch(c.ctx, 7, None, ctypes.byref(call.reads), call.ss.data_ptr()) == -2
    c.synchronize()
    untouched(call)
