"""tests/span_frames.py against the CPU oracle and against itself: the builder's reads have exactly the stream they were built for
(the oracle's svb encoder says so), span_plan keeps its invariants around every constant of the cut, and the catalogue holds what
tests/test_gpu_span_frames.py relies on -- every seam on both sides per launch kind, every content class, no repeat in any data region
that is not flagged -- counted here, from the oracle and numpy alone, so the device tests cannot shrink unnoticed."""
import numpy as np
import pytest

import oracle_lib as O
import sequences_ref as S
import span_frames as F

ROWS = pytest.mark.parametrize("row", F.rows(), ids=[r.name for r in F.rows()])


def test_the_constants():
    assert (F.SPAN_BLOCK, F.SPAN_BYTES, F.SHSPAN_BYTES, F.SHSPAN_MIN_REGION, F.SHSPAN_BATCH_FROM) == (16384, 32768, 8192, 16384, 20 << 20)
    assert (F.SPLIT_MIN, S.KEYSPAN_SHARED, S.KEYSPAN, S.KEYSPAN_LARGE_FROM) == (2048, 4096, 8192, 1 << 20)
    assert (F.SMALL_BATCH_MIN_AVG, F.TINY_DECODE_MIN_AVG) == (64 << 10, 8 << 10)


@pytest.mark.parametrize("T,a", [(16000, 383), (16000, 384), (16000, 385), (8192, 8192), (5, 0)])
def test_read_of_sets_the_stream_to_the_byte(T, a):
    rng = np.random.default_rng(T + a)
    codes = np.zeros(T, np.int64)
    codes[rng.permutation(T)[:a]] = 1
    data = rng.integers(1, 256, T + a).astype(np.uint8)
    x = F.read_of(codes, data)
    assert x.dtype == np.int16 and len(x) == T
    assert O.svb_compress(x, 2, True).tobytes() == F.stream_of(codes, data).tobytes()
    assert len(F.control_bytes(codes)) == (T + 3) // 4


@ROWS
def test_every_row_has_the_stream_it_was_built_for(row):
    want = O.svb_compress(row.read, row.opts[1], row.opts[0])
    assert not isinstance(want, int) and want.tobytes() == F.stream_of(row.codes, row.data).tobytes()
    assert len(want) == row.N == row.K + row.D and row.T == len(row.read)
    assert row.K == (F.key_bytes(row.N, row.T)) and (row.K == (row.T + 3) // 4 or row.N < F.SPLIT_MIN)
    assert row.read.dtype == {2: np.int16, 1: np.int8, 4: np.uint32}[row.opts[1]]


@ROWS
def test_the_oracle_round_trips_every_row(row):
    oo = O.options(*row.opts)
    f = O.compress(row.read, oo)
    assert not isinstance(f, int)
    back = O.decompress(f, row.read.nbytes, oo)
    assert not isinstance(back, int) and back.tobytes() == row.read.tobytes()


def _sweep():
    ks = sorted({k + e for k in (0, 1, 400, 4096, 8192, 12288, 16384, 3 * 4096) for e in (-1, 0, 1) if k + e >= 0})
    ds = sorted({d + e for d in (1, 2048, 8192, 16384, 24576, 32768, 40960, 65536, 65792, 98304) for e in (-1, 0, 1) if d + e >= 1})
    for K in ks:
        for D in ds:
            yield K + D, K
    for K in (S.KEYSPAN_LARGE_FROM - 1, S.KEYSPAN_LARGE_FROM, S.KEYSPAN_LARGE_FROM + 1):
        yield K + 100000, K


@pytest.mark.parametrize("shared_launch", [True, False])
def test_span_plan_invariants(shared_launch):
    assert F.span_plan(0, 0, shared_launch) == [F.Span(0, 0, "data", False, False)]
    seen = 0
    for N, K in _sweep():
        plan = F.span_plan(N, K, shared_launch)
        D = N - K
        assert plan[0].r0 == 0 and plan[-1].r1 == N
        assert all(a.r1 == b.r0 for a, b in zip(plan, plan[1:])) and all(s.r0 < s.r1 for s in plan), (N, K)       # a tiling of [0, N)
        keys = [s for s in plan if s.region == "key"]
        data = [s for s in plan if s.region == "data"]
        assert plan == keys + data and [(s.r0, s.r1) for s in keys] == S.key_spans(K, shared=shared_launch)
        assert (keys[-1].r1 if keys else 0) == K
        shared = shared_launch and K != 0 and D >= 16384
        assert all(s.shared == shared for s in data) and not any(s.shared or s.tree for s in keys)
        assert [s.tree for s in data] == [shared and t == 0 for t in range(len(data))]
        limit = 8192 if shared else 32768
        sizes = [s.r1 - s.r0 for s in data]
        assert max(sizes) <= limit and max(sizes) - min(sizes) <= 1 and len(data) == -(-D // limit), (N, K)       # evenly, none above the limit
        klimit = 4096 if shared_launch else (16384 if K >= 1 << 20 else 8192)
        assert all(s.r1 - s.r0 <= klimit for s in keys) and len(keys) == -(-K // klimit)
        assert len(plan) == F.span_count(N, K, shared_launch)
        for s in data:
            b = F.block_sizes(s.r1 - s.r0)
            assert sum(b) == s.r1 - s.r0 and max(b) <= 16384 and max(b) - min(b) <= 1 and len(b) == -(-(s.r1 - s.r0) // 16384)
        ix = F.index_of(plan, N)
        assert (ix is None) == (len(plan) == 1) and (ix is None or ix == (shared, [s.r0 for s in plan]))
        seen += 1
    assert seen >= 500


def test_key_bytes_and_header_length():
    assert F.key_bytes(2047, 1600) == 0 and F.key_bytes(2048, 1600) == 400 and F.key_bytes(2048, 9000) == 0
    assert [F.header_len(n) for n in (0, 255, 256, 65791, 65792)] == [6, 6, 7, 7, 9]


def test_parse_reads_what_the_statement_writes():
    """a frame put together by hand: two raw blocks and an RLE block, a checkpoint trailer and an index"""
    body = np.concatenate([np.array([F.ZSTD_MAGIC], "<u4").view(np.uint8), np.array([0x20, 9], np.uint8),
                           np.array([3 << 3, 0, 0, 1, 2, 3], np.uint8), np.array([(4 << 3) | 2, 0, 0, 7], np.uint8), np.array([(2 << 3) | 1, 0, 0, 5, 6], np.uint8)])
    cp = F.trailer(F.CP_MAGIC, [5])
    ix = F.trailer(F.IDX_MAGIC, [2 | 1 << 31, 6, 0, 12, 3])
    p = F.parse(np.concatenate([body, cp, ix]))
    assert p.body.tobytes() == body.tobytes() and p.checkpoints.tobytes() == cp.tobytes() and p.flag is True
    assert p.entries == [(6, 0), (12, 3)] and p.header_len == 6 and p.content_size == 9
    assert p.blocks == [(6, 0, None, 3), (12, 1, None, 4), (16, 0, None, 2)] and p.spans == [[(0, None, 3)], [(1, None, 4), (0, None, 2)]]
    q = F.parse(body)
    assert q.checkpoints is None and q.entries is None and q.flag is None and q.blocks == p.blocks


# ---- what the catalogue must contain ------------------------------------------------------------------------------------------------------
def _has(pred):
    return any(pred(r) for r in F.rows())


def test_every_seam_on_both_sides():
    rows = F.rows()
    i16 = [r for r in rows if r.opts == F.I16]
    ns = sorted(r.N for r in rows)
    assert {2047, 2048, 2049} <= set(ns) and {0, 2} <= set(ns)                                   # the control-byte region appears; empty, one sample
    for N in (65791, 65792):                                                                       # fhl under an index, in both launch kinds
        assert any(r.N == N and len(F.span_plan(r.N, r.K, sh)) > 1 for r in i16 for sh in (True,)) and any(r.N == N and len(F.span_plan(r.N, r.K, False)) > 1 for r in rows)
    assert _has(lambda r: r.N > 65792 and r.K)
    # shared launch: D around SHSPAN_MIN_REGION at K ~ 4000 (unshared one span, shared two, shared three), D around 8192 m, K around 4096 m
    for D, n, sh in ((16383, 1, False), (16384, 2, True), (16385, 3, True)):
        got = [F.span_plan(r.N, r.K, True) for r in i16 if r.D == D and 3900 <= r.K <= 4100]
        assert got and all([s.shared for s in p if s.region == "data"] == [sh] * n for p in got), D
    for m in (3, 4):
        for e in (-1, 0, 1):
            assert any(r.D == 8192 * m + e and r.K for r in i16), (m, e)
    for K in (4096, 4097, 8192, 8193):
        assert any(r.K == K and r.D >= 16384 for r in i16), K
    # unshared launch (VBZ_HIP_SHARED_TABLES=0): K = 8192 / 8193; D = 32 768 / 32 769 one span or two; D = 16 384 / 16 385 one block or two
    for opts in (F.I16, F.U32):
        sel = [r for r in rows if r.opts == opts]
        for D, n in ((32768, 1), (32769, 2)):
            assert any(r.D == D and sum(s.region == "data" for s in F.span_plan(r.N, r.K, False)) == n for r in sel), (opts, D)
        for D, n in ((16384, 1), (16385, 2)):
            assert any(r.D == D and len(F.block_sizes(r.D)) == n and sum(s.region == "data" for s in F.span_plan(r.N, r.K, False)) == 1 for r in sel), (opts, D)
    assert all(not F.launch_shared(r.opts) for r in rows if r.opts == F.U32) and F.launch_shared(F.I8) and F.launch_shared(F.I16)
    assert not F.launch_shared(F.I16, shared_tables=False)
    # a read below the minimum inside a shared launch brings its own table: no bit 31
    assert any(r.K and r.D < 16384 and F.index_of(F.span_plan(r.N, r.K, True), r.N)[0] is False for r in i16)
    i8 = sorted(r.D for r in rows if r.opts == F.I8)
    assert i8 == [16383, 16384] and all(r.D == r.T for r in rows if r.opts == F.I8)
    big = F.large_key_rows()
    assert [r.K for r in big] == [(1 << 20) - 1, 1 << 20]
    assert all(O.svb_compress(r.read, 2, True).tobytes() == F.stream_of(r.codes, r.data).tobytes() for r in big)
    assert [max(s.r1 - s.r0 for s in F.span_plan(r.N, r.K, False) if s.region == "key") > 8192 for r in big] == [False, True]


def test_every_content_class():
    rows = F.rows()
    by = {}
    for r in rows:
        by.setdefault(r.content, []).append(r)
    assert set(by) == {"none", "skewed", "uniform", "rare first", "uniform span", "once", "constant span", "two symbols", "one value", "gradient"}
    for r in rows:
        if r.content in ("none", "skewed", "gradient"):
            continue
        plan = F.span_plan(r.N, r.K, True)
        data = [s for s in plan if s.region == "data"]
        assert 4 <= len(data) <= 6 and all(s.shared for s in data) and not r.codes.any(), r.name
    assert sorted(r.raw_spans for r in by["uniform span"]) == [(1,), (2,), (4,)]
    hist = lambda b: np.bincount(b, minlength=256)
    for r in by["uniform span"] + by["uniform"]:                     # the spans said to be incompressible hold (nearly) every byte value
        data = [s for s in F.span_plan(r.N, r.K, True) if s.region == "data"]
        for t in r.raw_spans:
            h = hist(r.data[data[t].r0 - r.K : data[t].r1 - r.K])
            assert (h > 0).sum() >= 250 and h.max() < 80, r.name
    (r,) = by["rare first"]
    data = [s for s in F.span_plan(r.N, r.K, True) if s.region == "data"]
    h = hist(r.data)
    assert (h > 0).sum() == 256
    first = r.data[: data[0].r1 - r.K]
    assert float(np.mean(-np.log2(h[first] / len(r.data)))) > 9.5     # the tree span's bytes cost ~10 bits each under the region's table
    assert not set(first.tolist()) & set(r.data[data[1].r0 - r.K :].tolist())
    (r,) = by["once"]
    data = [s for s in F.span_plan(r.N, r.K, True) if s.region == "data"]
    once = np.flatnonzero(hist(r.data) == 1)
    assert any(data[-1].r0 - r.K <= int(np.flatnonzero(r.data == v)[0]) for v in once)
    (r,) = by["constant span"]
    data = [s for s in F.span_plan(r.N, r.K, True) if s.region == "data"]
    assert len(set(r.data[data[2].r0 - r.K : data[2].r1 - r.K].tolist())) == 1 and len(set(r.data[: data[1].r1 - r.K].tolist())) > 100
    assert len(set(by["two symbols"][0].data.tolist())) == 2 and len(set(by["one value"][0].data.tolist())) == 1


def test_the_gradient_row_crosses_the_fallbacks_bound():
    """under an optimal code for its region the spans behind the flat ones cost from well below their size to well above it, in steps far
    below the 64 bytes that variant 3 of the fallback's test would let through"""
    (r,) = [r for r in F.rows() if r.content == "gradient"]
    data = [s for s in F.span_plan(r.N, r.K, True) if s.region == "data"]
    assert len(data) == F.GRADIENT_SPANS and all(s.r1 - s.r0 == F.GRADIENT_SPAN and s.shared for s in data)
    cost = np.array(F.gradient_costs(r.data)) - F.GRADIENT_SPAN
    flat = F.GRADIENT_FLAT
    assert cost[:flat].max() < -500 and cost[flat] < -100 and cost[-1] > 150
    assert np.abs(np.diff(cost[flat:])).max() < 50 and float(np.mean(np.diff(cost[flat:]))) < 25


def test_control_byte_content_rows():
    rows = [r for r in F.rows() if "keys" in r.tags]
    assert len(rows) == 7 and all(r.K == 8193 for r in rows)
    key = {r.name: F.control_bytes(r.codes) for r in rows}
    assert not key["keys all zero"].any() and key["keys without a zero"].all()
    runs = S.runs_ref(key["keys in zero runs"][:2731])[0]
    assert len(runs) >= 4 * S.CP_MIN_SPACING                        # sequences enough in the first key span for checkpoints
    seams = {S.key_spans(8193, shared=True)[0][1], S.key_spans(8193, shared=False)[0][1]}
    assert seams == {2731, 4096}
    for r in rows:
        if len(r.tags) < 3:
            continue
        k, seam = key[r.name], r.tags[2]
        zero = np.flatnonzero(k == 0)
        run = [z for z in zero if abs(int(z) - seam) <= 700]
        if r.tags[1] == "run ends on":
            assert k[seam - 600 : seam].max() == 0 and k[seam] != 0, r.name
        else:
            assert k[seam - 300 : seam + 300].max() == 0 and k[seam + 300] != 0 and k[seam - 301] != 0, r.name
        assert len(run) >= 600
    assert {(r.tags[1], r.tags[2]) for r in rows if len(r.tags) == 3} == {(w, s) for w in ("run ends on", "run crosses") for s in seams}


def _windows(data):
    """the 16-byte windows of a region, one row each"""
    return np.lib.stride_tricks.sliding_window_view(np.ascontiguousarray(data), 16) if len(data) >= 16 else np.zeros((0, 16), np.uint8)


def test_only_the_three_named_classes_may_match():
    rows = F.rows()
    assert {r.content for r in rows if r.may_match} == {"constant span", "two symbols", "one value"}
    for r in rows:
        if r.may_match:
            continue
        w = _windows(r.data)
        seen = set(map(bytes, w))
        assert len(seen) == len(w), (r.name, len(w) - len(seen))       # no 16-byte window of the data region occurs twice
