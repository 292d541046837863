"""GPU tests (-m gpu) of the span entropy stage of the large-read path: every row of tests/span_frames.py -- one read per
seam of the cut and per kind of block -- is written by five contexts (six writers) and every frame is held to the statement, exactly: the index's
content offsets are span_plan's, bit 31 is the statement's, the frame offsets are block starts, entry 0 is the header's length, a frame
of one span has no index and a frame of several must have one; the blocks under every data span are of the kind the statement gives
(tree, treeless, raw, RLE) and no span but the tree span exceeds its content by more than 3 bytes per block.  Then every frame is read
by the oracle (libzstd) and by seven device readers, and the indexed ones must be decoded span by span (decode_span_paths).  The
writer's three capacity checks and the two call-level seams (20 MB of stream bound, read 1024 / 1025 of a call) follow.

The rule the (1, 1) check forced into the open: a call decodes on the large-read path by its shape (vbz_api.hip, use_segments: for up
to 64 reads, 8 KB of output per read and more), so an indexed frame of less -- the rows around N = 2048 -- is read by the one-wavefront
decoder in the default context; those frames are asked of the VBZ_HIP_SEGMENTED=1 context instead, where they too must report (1, 1).

Counts and times of the first run on an MI355X (43 rows: 26 geometry, 9 data content, the gradient, 7 control-byte content; + 2 of 8 MB):
  writer               one wavefront  one span  matcher's  indexed
  default                   22            0         1         20
  segmented                  0            3         1         39      (and the same reversed)
  own tables                 0            3         1         39
  no repeats                 0            3         0         40
  no trailers: 43 plain frames, each the body of the default writer's
  259 frames in all; 177 indexed ones decoded alone, all (1, 1), 8 of them in the segmented context (N = 2048 / 2049); every frame read
  by the oracle, by both one-wavefront contexts, without its index, without any trailer, and by the entropy stage alone in roomy and in
  exact slots.  Gradient row: 10 spans treeless with 183 ... 25 bytes to spare, then 14 raw.  Capacity rows (body, checkpoints, index):
  32 891 / 0 / 80, 34 692 / 0 / 80, 28 025 / 32 / 80.  Calls of 1031 reads: bound 20 971 456 (flag set) and 20 971 528 (clear).
  Module 3.6 s: the 8 MB pair 0.54 s, the default writer 0.38 s, the (1, 1) test 0.11 s, each 1031-read call 0.09 s, nothing else above 0.05 s.
  One-line variants of zstd_encode.hip, new tests failing / of the 19 older large-read tests run against them: `>` for `>=` in span_cut
  4 / 0; `<=` in fhl 5 / 0; the fallback 64 bytes later 5 / 0; the index without bit 31 6 / 1."""
import ctypes
import time

import numpy as np
import pytest

import oracle_lib as O
import span_frames as F
import typed_support as T
from vbz_compression_amd import _lib

pytestmark = pytest.mark.gpu

CANARY = 0x5A
SEG = {"VBZ_HIP_SEGMENTED": 1}
# writer: (the context's knobs, one row per call, rows reversed)
WRITERS = {
    "default": ({}, True, False),
    "segmented": (SEG, False, False),
    "segmented reversed": (SEG, False, True),
    "own tables": (dict(SEG, VBZ_HIP_SHARED_TABLES=0), False, False),
    "no repeats": (dict(SEG, VBZ_HIP_LONG_REPEATS=0), False, False),
    "no trailers": ({"VBZ_HIP_TRAILERS": 0}, True, False),
}


def options(row):
    return _lib.CompressionOptions(*row.opts)


def cap_of(c, row):
    return c.L.vbz_max_compressed_size(int(row.read.nbytes), ctypes.byref(options(row)))


def write(c, rows, caps=None, **kw):
    """the frames of rows of one type in one call -> Stage"""
    assert len({r.opts for r in rows}) == 1
    o = options(rows[0])
    return T.run_stage(c, lambda c, *a: c.compress(*a, o), [r.read for r in rows], caps or [cap_of(c, r) for r in rows], **kw)


def read_back(c, rows, frames, **kw):
    o = options(rows[0])
    return T.run_stage(c, lambda c, *a: c.decompress(*a, o), frames, [r.read.nbytes for r in rows], **kw)


def by_type(rows):
    out = {}
    for r in rows:
        out.setdefault(r.opts, []).append(r)
    return list(out.values())


_written = {}


def written(writer):
    """[(row, frame, on the span path)] of one writer, made once"""
    if writer not in _written:
        knobs, per_row, rev = WRITERS[writer]
        c = T.codec(**knobs)
        out = []
        for group in by_type(F.rows()[::-1] if rev else F.rows()):
            for rows in ([[r] for r in group] if per_row else [group]):
                st = write(c, rows)
                # vbz_api.hip:465-471 (use_segments, encode): forced, or 64 KB and more of raw bytes per read in a call of up to 96 MB
                spans = "VBZ_HIP_SEGMENTED" in knobs or st.src_bytes // len(rows) >= F.SMALL_BATCH_MIN_AVG
                for r, f in zip(rows, st.out):
                    assert not isinstance(f, int), (writer, r.name, hex(f))
                    assert len(f) <= cap_of(c, r), (writer, r.name)
                    out.append((r, f, spans))
        _written[writer] = out
    return _written[writer]


def all_frames():
    return [(w, r, f) for w in WRITERS for r, f, _ in written(w)]


def span_bytes(blocks):
    return sum(3 + (1 if b[0] == 1 else b[2]) for b in blocks)


def hold_to_statement(row, frame, shared, matcher_allowed):
    """one frame of the span path against span_plan -> "one span", "matcher" or "indexed" """
    p = F.parse(frame)
    assert p.content_size == row.N and p.header_len == F.header_len(row.N), row.name
    plan = F.span_plan(row.N, row.K, shared)
    want = F.index_of(plan, row.N)
    if want is None:
        assert p.entries is None, (row.name, "a frame of one span carries no index")
        return "one span"
    if p.entries is None:
        assert row.may_match and matcher_allowed, (row.name, "a frame of %d spans without its index" % len(plan))
        return "matcher"
    starts = {b[0] for b in p.blocks}
    assert [e[1] for e in p.entries] == want[1], (row.name, [e[1] for e in p.entries], want[1])
    assert p.flag == want[0], (row.name, p.flag)
    assert p.entries[0][0] == p.header_len and all(e[0] in starts for e in p.entries), row.name
    for j, (s, kind, blocks) in enumerate(zip(plan, F.expected_kinds(row, plan), p.spans)):
        size = s.r1 - s.r0
        what = (row.name, j, kind, blocks)
        if kind == "key":
            continue
        even = F.block_sizes(size)
        if kind == "own or raw" and blocks[0][0] == 0:
            assert blocks == [(0, None, size)], what
        elif kind in ("tree", "own", "own or raw"):
            assert [b[:2] for b in blocks] == [(2, 2)] + [(2, 3)] * (len(even) - 1), what
        elif kind == "treeless":
            assert [b[:2] for b in blocks] == [(2, 3)] * len(even), what
        elif kind == "raw":
            assert blocks == ([(0, None, n) for n in even] if s.shared else [(0, None, size)]), what
        elif kind == "either":
            assert blocks == [(0, None, n) for n in even] or [b[:2] for b in blocks] == [(2, 3)] * len(even), what
        elif kind == "rle":
            assert blocks == ([(1, None, n) for n in even] if s.shared else [(1, None, size)]), what
        if s.shared and not s.tree:     # the contract in zstd_span_pack_kernel's comment (zstd_encode.hip:2926-2929, 2950)
            assert span_bytes(blocks) <= size + 3 * len(blocks), what
        if row.content == "rare first" and s.tree:
            assert span_bytes(blocks) > size + 3 * len(blocks), what   # 10 bits per byte: the tree span cannot fall back, and did not
    return "indexed"


@pytest.mark.parametrize("writer", list(WRITERS))
def test_every_frame_is_the_statements(writer):
    knobs = WRITERS[writer][0]
    shared_tables = knobs.get("VBZ_HIP_SHARED_TABLES", 1) != 0
    seen = {"one wavefront": 0, "one span": 0, "matcher": 0, "indexed": 0, "plain": 0}
    for row, frame, spans in written(writer):
        if knobs.get("VBZ_HIP_TRAILERS", 1) == 0:
            p = F.parse(frame)
            assert p.entries is None and p.checkpoints is None and len(p.body) == len(frame), row.name      # one plain frame
            (same,) = [f for r, f, _ in written("default") if r.name == row.name]
            assert F.parse(same).body.tobytes() == frame.tobytes(), row.name                               # ... of the same blocks
            seen["plain"] += 1
        elif not spans:
            assert F.parse(frame).entries is None, row.name
            seen["one wavefront"] += 1
        else:
            seen[hold_to_statement(row, frame, F.launch_shared(row.opts, shared_tables), knobs.get("VBZ_HIP_LONG_REPEATS", 1) != 0)] += 1
    print(writer, seen)
    if "VBZ_HIP_SEGMENTED" in knobs:
        n = sum(len(F.span_plan(r.N, r.K, F.launch_shared(r.opts, shared_tables))) > 1 for r in F.rows())
        assert seen["indexed"] + seen["matcher"] == n and seen["matcher"] <= 3 and seen["one span"] == len(F.rows()) - n
    if writer == "default":
        assert seen["indexed"] + seen["matcher"] >= 12 and seen["one wavefront"] >= 20


def test_the_fallbacks_bound_is_met_from_both_sides():
    """the gradient row: behind the flat spans the first spans stay treeless, the last are stored raw, and the costliest treeless one is
    within 64 bytes of the bound -- a fallback that let a span through that much later would show in hold_to_statement"""
    (hit,) = [(r, f) for r, f, _ in written("segmented") if r.content == "gradient"]
    p = F.parse(hit[1])
    spans = p.spans[-F.GRADIENT_SPANS :][F.GRADIENT_FLAT :]
    raw = [b[0][0] == 0 for b in spans]
    room = [F.GRADIENT_SPAN + 3 - span_bytes(b) for b in spans if b[0][0] == 2]
    print("gradient: raw", "".join("r" if x else "t" for x in raw), "room of the treeless spans", room)
    assert sum(raw) >= 3 and len(room) >= 3 and not raw[0] and raw[-1]
    assert 0 <= min(room) < 64, room


def same(got, row):
    return not isinstance(got, int) and got.tobytes() == row.read.tobytes()


def test_the_oracle_reads_every_frame():
    for w, r, f in all_frames():
        assert same(O.decompress(f, r.read.nbytes, O.options(*r.opts)), r), (w, r.name)


def test_indexed_frames_decode_span_by_span():
    """every frame alone in a call of the default context: the read comes back, and an indexed frame reports (1, 1); below the decode
    shape rule's 8 KB of output the default context takes the one-wavefront decoder, and the VBZ_HIP_SEGMENTED=1 context is asked"""
    c, cs = T.codec(), T.codec(**SEG)
    by_spans = asked_segmented = 0
    for w, r, f in all_frames():
        st = read_back(c, [r], [f])
        assert same(st.out[0], r), (w, r.name)
        if F.parse(f).entries is None:
            continue
        paths = c.decode_span_paths()
        # vbz_api.hip:465-471 (use_segments, decode): 64 reads or fewer of 8 KB and more each
        if st.dst_bytes >= F.TINY_DECODE_MIN_AVG:
            assert paths == (1, 1), (w, r.name, paths)
        else:
            assert paths == (0, 0) and r.N < 4096, (w, r.name, paths)
            assert same(read_back(cs, [r], [f]).out[0], r) and cs.decode_span_paths() == (1, 1), (w, r.name)
            asked_segmented += 1
        by_spans += 1
    print("indexed frames decoded by spans:", by_spans, "of them in the segmented context:", asked_segmented)
    assert by_spans >= 140 and asked_segmented >= 8


@pytest.mark.parametrize("knobs", [{"VBZ_HIP_SEGMENTED": 0}, {"VBZ_HIP_SEGMENTED": 0, "VBZ_HIP_FAST_DECODE": 0}], ids=["one wavefront", "no fast decode"])
def test_the_one_wavefront_decoders_read_every_frame(knobs):
    c = T.codec(**knobs)
    frames = all_frames()
    for opts in (F.I16, F.I8, F.U32):
        sel = [(w, r, f) for w, r, f in frames if r.opts == opts]
        st = read_back(c, [r for _, r, _ in sel], [f for _, _, f in sel])
        for (w, r, _), got in zip(sel, st.out):
            assert same(got, r), (w, r.name, knobs)


def test_frames_without_their_trailers():
    """the index cut off, then both trailers: the default context reads the same samples"""
    c = T.codec()
    frames = [(w, r, f) for w, r, f in all_frames() if len(F.parse(f).body) != len(f)]
    assert len(frames) >= 140
    for opts in (F.I16, F.I8, F.U32):
        sel = [(w, r, f) for w, r, f in frames if r.opts == opts]
        rows = [r for _, r, _ in sel]
        cut = []
        for _, _, f in sel:
            p = F.parse(f)
            cut.append((f[: len(p.body) + (len(p.checkpoints) if p.checkpoints is not None else 0)], p.body))
        for k in (0, 1):
            st = read_back(c, rows, [np.ascontiguousarray(x[k]) for x in cut])
            for (w, r, _), got in zip(sel, st.out):
                assert same(got, r), (w, r.name, ("index cut off", "both trailers cut off")[k])


def test_the_entropy_stage_alone_roomy_and_exact_slots():
    """vbz_gpu_zstd_decompress_batch under VBZ_HIP_SEGMENTED=1, all frames in one call: slots with room, then slots of exactly the content,
    laid without gaps, a canary behind the last -- a span with sequences has no stripe there and hands its frame to the ordinary decoder"""
    c = T.codec(**SEG)
    frames = all_frames()
    streams = {r.name: F.stream_of(r.codes, r.data) for r in F.rows()}
    for caps, align, pad in ([r.N + 64 for _, r, _ in frames], 64, 32), ([r.N for _, r, _ in frames], 1, 0):
        st = T.run_stage(c, lambda c, *a: c.zstd_decompress(*a), [f for _, _, f in frames], caps, align=align, pad=pad, fill=CANARY)
        for (w, r, _), got in zip(frames, st.out):
            assert not isinstance(got, int) and got.tobytes() == streams[r.name].tobytes(), (w, r.name, pad)
        end = st.off[-1] + caps[-1]
        assert (st.host[end:] == CANARY).all(), "written behind the last slot"
        if pad == 0:
            assert end == sum(caps)
        else:
            for o, cap, nxt in zip(st.off, caps, st.off[1:] + [len(st.host)]):
                assert (st.host[o + cap : nxt] == CANARY).all(), "written behind a slot"


def test_the_key_spans_double_at_two_to_the_twenty():
    """K = 2^20 - 1 / 2^20 in a launch without shared tables (KEYSPAN_LARGE_FROM): 128 key spans of 8 KB, then 64 of 16 KB"""
    c = T.codec(**dict(SEG, VBZ_HIP_SHARED_TABLES=0))
    rows = F.large_key_rows()
    st = write(c, rows)
    for r, f in zip(rows, st.out):
        assert hold_to_statement(r, f, False, False) == "indexed"
        assert same(O.decompress(f, r.read.nbytes, O.options(*r.opts)), r), r.name
    nkeys = [sum(e[1] < r.K for e in F.parse(f).entries) for r, f in zip(rows, st.out)]
    assert nkeys == [128, 64], nkeys
    c0 = T.codec()
    for r, f in zip(rows, st.out):
        assert same(read_back(c0, [r], [f]).out[0], r) and c0.decode_span_paths() == (1, 1), r.name


# ---- the writer's capacity checks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["K=8192 T=32769 D=40000", "one uniform span in the middle", "keys in zero runs"])
def test_capacity_seams_of_the_writer(name):
    """zstd_span_finish_kernel (zstd_encode.hip:3018-3049): below the body's size the read is refused; from it on the frame is the same
    body with the trailers that fit, the checkpoint trailer first, then the index behind whatever stands"""
    c = T.codec(**SEG)
    (row,) = [r for r in F.rows() if r.name == name]
    (other,) = [r for r in F.rows() if r.name == "D=16384 T=16000 D=16385"]
    rows = [other] + [row] * 6 + [other]
    roomy = write(c, rows, fill=CANARY)
    assert all(f.tobytes() == roomy.out[1].tobytes() for f in roomy.out[2:7])
    p = F.parse(roomy.out[1])
    assert p.entries is not None and len(p.entries) >= 6
    B, C, I = len(p.body), len(p.checkpoints) if p.checkpoints is not None else 0, 16 + 8 * len(p.entries)
    assert len(roomy.out[1]) == B + C + I
    index = roomy.out[1][B + C :]
    cps = roomy.out[1][B : B + C]
    room = cap_of(c, other)
    caps = [room, B - 1, B, B + C - 1, B + C, B + C + I - 1, B + C + I, room]
    st = write(c, rows, caps=caps, fill=CANARY)
    print(name, "B, C, I =", B, C, I)
    for k in (0, 7):
        assert st.out[k].tobytes() == roomy.out[k].tobytes(), "a neighbour in the same call changed"
    accepted = []
    for cap, f in list(zip(caps, st.out))[1:7]:
        if cap < B:
            assert f == _lib.VBZ_ZSTD_ERROR, (name, cap, f if isinstance(f, int) else len(f))
            continue
        assert not isinstance(f, int), (cap, hex(f))
        want, at = [p.body], B
        if at + C <= cap:
            want.append(cps)
            at += C
        if at + I <= cap:
            want.append(index)
        assert f.tobytes() == np.concatenate(want).tobytes(), (name, cap, len(f))
        accepted.append(f)
    assert len(accepted) >= 4 and (C == 0 or len({len(f) for f in accepted}) >= 3)
    if name == "keys in zero runs":
        assert C >= 16 + 4 * 4, C                                   # a checkpoint trailer of several words: all six capacities differ
    for o, cap, nxt in zip(st.off, caps, st.off[1:] + [len(st.host)]):
        assert (st.host[o + cap : nxt] == CANARY).all(), ("written behind a slot of", cap)
    back = read_back(c, [row] * len(accepted), accepted)
    for f, got in zip(accepted, back.out):
        assert same(got, row) and same(O.decompress(f, row.read.nbytes, O.options(*row.opts)), row), (name, len(f))


# ---- the call-level seams -------------------------------------------------------------------------------------------------------------------
def _call_rows(filler_samples):
    """1030 reads of 8192 two-byte samples (K = 2048, D = 16 384, N = 18 432: eight different ones in turn) and one filler read"""
    rng = np.random.default_rng(4605)
    eight = [F.row_of("two-byte %d" % k, F.I16, np.ones(8192, np.int64), F.skewed(rng, 16384, nonzero=True)) for k in range(8)]
    filler = F.row_of("filler", F.I16, np.zeros(filler_samples, np.int64), F.skewed(rng, filler_samples))
    return [eight[k % 8] for k in range(1030)] + [filler]


def _bound(filler_samples):
    """the bound on the stream bytes of the call of _call_rows as vbz_api.hip:570 has it for int16 zig-zag reads (9 / 8 of the raw arena, 96
    bytes a read, 256): only used to place the two calls either side of SHSPAN_BATCH_FROM -- what a call did is read from its frames"""
    arena = 1030 * 16384 + (2 * filler_samples + 63) // 64 * 64 + 128     # typed_support.arena's extent
    return (arena * 9 + 7) // 8 + 96 * 1031 + 256


@pytest.mark.parametrize("side", ["under", "over"])
def test_twenty_megabytes_of_stream_bound_and_the_plan_kernels_rounds(side):
    """A call of 1031 reads just under / just over SHSPAN_BATCH_FROM: all frames of the call agree on bit 31, every frame's geometry is
    span_plan(N, K, that flag) -- reads 1023 ... 1025 straddle the plan kernel's round of 1024 reads with its carried prefix --, the call
    under the bound shares tables and the call over it does not; 40 reads spread over the call decode, 1022 ... 1026 among them"""
    base = max(t for t in range(0, 2_000_000, 32) if _bound(t) < F.SHSPAN_BATCH_FROM)     # the longest filler that stays below the seam
    filler = base if side == "under" else base + 32
    assert (_bound(filler) < F.SHSPAN_BATCH_FROM) == (side == "under") and abs(_bound(filler) - F.SHSPAN_BATCH_FROM) <= 72
    rows = _call_rows(filler)
    c = T.codec(**SEG)
    t0 = time.perf_counter()
    st = write(c, rows)
    flags = set()
    for k, (r, f) in enumerate(zip(rows, st.out)):
        assert not isinstance(f, int), (k, hex(f))
        p = F.parse(f)
        assert p.entries is not None, k
        flags.add(p.flag)
        assert len(flags) == 1, ("read", k, "disagrees on bit 31")
        assert hold_to_statement(r, f, p.flag, False) == "indexed", k
    assert flags == {side == "under"}, (side, flags)
    pick = sorted(set(range(0, 1031, 30)) | set(range(F.PLAN_ROUND - 2, F.PLAN_ROUND + 3)) | {1030})
    assert len(pick) >= 40
    back = read_back(c, [rows[k] for k in pick], [st.out[k] for k in pick])
    for k, got in zip(pick, back.out):
        assert same(got, rows[k]), k
        assert same(O.decompress(st.out[k], rows[k].read.nbytes, O.options(*F.I16)), rows[k]), k
    print(side, "filler", filler, "bound", _bound(filler), "seconds", round(time.perf_counter() - t0, 2))
