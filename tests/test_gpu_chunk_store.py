"""The identity the chunk store of svb_kernels.hip rests on: a whole read, a sequence of POD5 rows and a range of a longer
read are ONE store.  A signal x of T samples goes into a canary-filled chunk arena three ways -- (a) as one read, (b) cut into POD5 rows,
(c) as the range [b, b + T) of a longer read y -- and every arena must hold pod5_reads_ref.chunk_rows(x, ...) bit for bit.

The shapes are the smallest at which the line store can go wrong: T around one and two lanes (8 samples), a wavefront (512) and its double;
chunks of one line, of two overlapping lines and of a wavefront; PAD, END with end_align 1 (the END chunk starts d = last % 8 != 0 samples
into a line: shifted lines) and END with end_align 8 (d = 0).  The row cuts put a row boundary at a line boundary (8), inside a line (13:
the row's last lane is `partial`), at lane 63's boundary (512), inside the END chunk's shifted lines (504, 520), in front of an empty
last row and in front of a last row of one sample.  Range begins 8 and 2 048 take the line path, 3 and 2 051 the element path; no read is
longer than 2 100 samples, so the begins past 2 000 carry the T up to 17 only."""
import numpy as np
import pytest

import pod5_ref as P
import pod5_reads_ref as PR
from typed_support import ELEM, PAD, Call, Frames, Run, check_chunks, codec, expect_results, sine_signal

pytestmark = pytest.mark.gpu

SIZES = [9, 15, 16, 17, 519, 520, 521, 1033]
CHUNKINGS = [(8, 8), (16, 8), (512, 504)]
MODES = [("pad", 0), ("end", 1), ("end", 8)]
DTYPES = ["f16", "f32"]
BEGINS = [8, 2048, 3, 2051]
MAX_READ = 2100
CUTS = [(8,), (13,), (8, 13), (512,), (504,), (520,), (504, 520)]


def row_lengths(T):
    """the ways x is cut into rows: every cut set that lies inside x, an empty last row, a last row of one sample"""
    shapes = [[T, 0], [T - 1, 1]]
    for cuts in CUTS:
        if cuts[-1] < T:
            edges = [0, *cuts, T]
            shapes.append([b - a for a, b in zip(edges, edges[1:])])
    return shapes


def end_chunk(T, L, S, ea):
    """(last, d) of the END chunk, or None when the read has one chunk"""
    starts = PR.chunk_starts(T, L, S, "end", ea)
    return (starts[-1], starts[-1] % 8) if len(starts) >= 2 else None


def test_the_shapes_reach_what_they_are_for():
    """(CPU arithmetic on the chosen shapes.)  Every cut lies in an END chunk that starts inside a line (d != 0) for some (T, L, S), and for
    T = 9, L = S = 8, end_align 1 the lane of the last sample has i0 < T <= i0 + d: its shifted line holds no sample and is the pad writer's."""
    for cut in (8, 13, 512, 504, 520, "T-1"):
        hits = []
        for T in SIZES:
            for L, S in CHUNKINGS:
                ec = end_chunk(T, L, S, 1)
                at = T - 1 if cut == "T-1" else cut
                if ec and ec[1] != 0 and ec[0] <= at < T and any(at in np.cumsum(s) for s in row_lengths(T)):
                    hits.append((T, L, S))
        assert hits, cut
    last, d = end_chunk(9, 8, 8, 1)
    i0 = (9 - 1) // 8 * 8
    assert d != 0 and i0 < 9 <= i0 + d, (last, d, i0)
    for b in BEGINS:
        assert any(T + b + 5 <= MAX_READ for T in SIZES), b


_inputs = {}


def inputs(c):
    """x per T; (a) the x as reads; (b) their rows as pod5 wrote them; (c) the y with their begins -- compressed once"""
    if "i" not in _inputs:
        rng = np.random.default_rng(23)
        xs = [sine_signal(rng, T) if k % 3 else rng.integers(-32768, 32768, T).astype(np.int16) for k, T in enumerate(SIZES)]
        opts = c.options(True, 2, 1, 1)
        whole = Frames(c, xs, opts)
        rows, first, of_rows = [], [], []
        for k, x in enumerate(xs):
            for lens in row_lengths(len(x)):
                first.append(len(rows))
                of_rows.append(k)
                at = np.concatenate([[0], np.cumsum(lens)])
                rows += [x[a:b] for a, b in zip(at, at[1:])]
        frames = [P.compress_row(r) for r in rows]
        ys, begins, of_ys = [], [], []
        for k, x in enumerate(xs):
            for b in BEGINS:
                if len(x) + b + 5 <= MAX_READ:
                    ys.append(np.concatenate([rng.integers(-32768, 32768, b).astype(np.int16), x, rng.integers(-32768, 32768, 5).astype(np.int16)]))
                    begins.append(b)
                    of_ys.append(k)
        _inputs["i"] = dict(xs=xs, whole=whole, rows=rows, first=first, frames=frames, of_rows=of_rows, ranged=Frames(c, ys, opts), begins=begins, of_ys=of_ys)
    return _inputs["i"]


@pytest.mark.parametrize("mode,ea", MODES, ids=lambda v: str(v))
@pytest.mark.parametrize("L,S", CHUNKINGS)
def test_read_rows_and_range_are_one_store(L, S, mode, ea):
    c = codec()
    I = inputs(c)
    xs = I["xs"]
    chunking = (L, S, mode, ea)
    rng = np.random.default_rng(L + ea)
    o, s = rng.uniform(-600, 600, len(xs)).astype(np.float32), rng.uniform(0.01, 2.5, len(xs)).astype(np.float32)
    for dtype in DTYPES:
        want = [PR.chunk_rows(x, L, S, mode, ea, o[k], s[k], PAD, dtype)[1] for k, x in enumerate(xs)]   # the reference, once
        # (a) one read each, the un-ranged call
        a = Run(I["whole"], chunking, dtype, offset=o, scale=s, ranges=False).check()
        got = a.bits()
        for k in range(len(xs)):
            assert np.array_equal(got[a.table[k] : a.table[k + 1]], want[k]), ("read", chunking, dtype, len(xs[k]))
        # (b) POD5 rows
        of = I["of_rows"]
        call = Call(c, I["frames"], [len(r) for r in I["rows"]], PR.bounds(I["first"], len(I["rows"])), dtype, chunking, offset=o[of], scale=s[of])
        assert call.chunk_call() == 0, c.L.vbz_gpu_last_error(c.ctx)
        expect_results(call, I["rows"], I["first"], ELEM[dtype])
        check_chunks(call, I["rows"], I["first"], chunking, list(zip(o[of], s[of])))
        got, cf = call.chunk_bits(), call.first_host
        for j, k in enumerate(of):
            assert np.array_equal(got[cf[j] : cf[j + 1]], want[k]), ("rows", chunking, dtype, len(xs[k]), j)
        # (c) a range of a longer read
        of, bg = I["of_ys"], I["begins"]
        r = Run(I["ranged"], chunking, dtype, bg, [b + len(xs[k]) for b, k in zip(bg, of)], offset=o[of], scale=s[of]).check()
        got = r.bits()
        for j, k in enumerate(of):
            assert np.array_equal(got[r.table[j] : r.table[j + 1]], want[k]), ("range", chunking, dtype, len(xs[k]), bg[j])
