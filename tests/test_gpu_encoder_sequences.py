"""The encoder's sequences and checkpoints held to the plain statement of tests/sequences_ref.py (-m gpu).

Every frame first decodes with libzstd to its stream.  Then oracle_lib.zstd_sequences lists what the frame holds -- every block's extent and
literals, every sequence's literal length, match length and offset, the decoder's state at the head of every sequence -- and that listing
is compared EXACTLY with what the statement says the encoder must have found: runs_ref for the control bytes (tokenise_runs, offset 1),
period_ref for the long-repeat matcher (explicit offset D), checkpoints_ref for the trailer.  A missed or shortened match still makes a
valid frame that round-trips and stays inside the ratio tests' band; here it is a failure.

How the regions reach the tokeniser.  The zstd stage on its own (gpu_util.zstd_compress, vbz_gpu_zstd_compress_batch) never tokenises: its
source is the caller's arena, which the tokeniser would rewrite in place, so the call passes no slot capacity and every control-byte region
leaves as raw or Huffman blocks -- measured: a region with three runs comes back as two raw blocks.  (So a test that feeds that call regions
full of runs, as test_gpu_parity.py's test_sequences_section_round_and_lane_boundaries does, never reaches the sequences section.)  The
tokeniser runs in the whole codec only, where the svb stream lies in the library's own slot.  The regions are therefore built as READS:
uint32 values without delta or zig-zag (options False, 4, 1, 0), four values per control byte, two bits each = the value's byte count - 1,
so EVERY byte string is some read's control-byte region [0, K), K = len(values) / 4; the values are random inside their byte count (random
data bytes: no period for the matcher, no runs) but for the first, whose low byte -- the first data byte, the byte behind the region's
last -- can be chosen.  The slot is the library's own (the svb bound of the read), as for every caller.

Builds (knobs are read when a context is created: typed_support.codec):
  staged      VBZ_HIP_SEGMENTED=0 VBZ_HIP_ROUTING=0: zstd_plan_kernel tokenises, zstd_pack_kernel writes (the default path)
  one_launch  the same and VBZ_HIP_STAGED_ENCODE=0: zstd_encode_kernel does both
  spans       VBZ_HIP_SEGMENTED=1: the control bytes in spans of at most KEYSPAN bytes (sequences_ref.key_spans), a block each, every one
              tokenised as if nothing stood in front of it
"""
import functools

import numpy as np
import pytest

import entropy_host as E
import oracle_lib as O
import sequences_ref as S
import typed_support as T
from vbz_compression_amd import _lib

pytestmark = pytest.mark.gpu

RMIN, RPER, BLOCK_MAX = S.RMIN, S.RPER, S.BLOCK_MAX
CP_MAGIC = 0x184D2A5B
BUILDS = {
    "staged": dict(VBZ_HIP_SEGMENTED=0, VBZ_HIP_ROUTING=0),
    "one_launch": dict(VBZ_HIP_SEGMENTED=0, VBZ_HIP_ROUTING=0, VBZ_HIP_STAGED_ENCODE=0),
    "spans": dict(VBZ_HIP_SEGMENTED=1),
}
WHOLE = ("staged", "one_launch")   # the builds that code a control-byte region of up to a block as ONE block
# RFC 8878 3.1.1.3.2.1.1: the baselines of the literal-length and match-length codes
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
assert len(LL_BASE) == 36 and len(ML_BASE) == 53


# ---- control-byte regions ------------------------------------------------------------------------------------------------------------
def noise(rng, n, last=None):
    """n bytes of which no two neighbours are equal (and the first differs from `last`): no run at all"""
    d = rng.integers(1, 256, n)
    return ((0 if last is None else int(last)) + np.cumsum(d)).astype(np.uint8) if n else np.zeros(0, np.uint8)


def put_run(x, start, length, value):
    """a run of exactly `length` bytes of `value` at x[start:]: the bytes on both sides are made to differ from it"""
    assert 0 <= start and start + length <= len(x)
    x[start : start + length] = value
    if start > 0 and x[start - 1] == value:
        x[start - 1] = value ^ 0x80
    if start + length < len(x) and x[start + length] == value:
        x[start + length] = value ^ 0x80
    return x


def region_of(rng, pairs, tail):
    """control bytes whose sequences are exactly `pairs` (literal length >= 1, match length >= RMIN - 1) and `tail` literals behind them"""
    parts, last = [], None
    for ll, ml in pairs:
        assert ll >= 1 and ml >= RMIN - 1
        parts.append(noise(rng, ll - 1, last))
        last = parts[-1][-1] if ll > 1 else last
        v = np.uint8(((0 if last is None else int(last)) + int(rng.integers(1, 256))) & 0xFF)
        parts.append(np.full(ml + 1, v, np.uint8))
        last = v
    parts.append(noise(rng, tail, last))
    x = np.concatenate(parts)
    got = S.runs_ref(x)
    assert got[0] == list(pairs) and len(got[1]) == sum(ll for ll, _ in pairs) + tail
    return x


def read_of(rng, ctl, first_data=None):
    """uint32 values (no delta, no zig-zag) whose svb stream begins with the control bytes `ctl`; first_data: the stream's first data byte"""
    codes = ((ctl[:, None] >> np.array([0, 2, 4, 6], np.uint8)) & 3).reshape(-1).astype(np.uint64)
    lo = np.where(codes == 0, np.uint64(0), np.uint64(1) << (np.uint64(8) * codes))
    hi = np.uint64(1) << (np.uint64(8) * (codes + np.uint64(1)))
    v = lo + rng.integers(0, 1 << 62, len(codes)).astype(np.uint64) % (hi - lo)
    if first_data is not None:
        v[0] = (v[0] & ~np.uint64(0xFF)) | np.uint64(first_data)
    return v.astype(np.uint32)


class Case:
    def __init__(self, name, rng, ctl, first_data=None):
        self.name, self.ctl, self.K = name, np.ascontiguousarray(ctl, np.uint8), len(ctl)
        self.read = read_of(rng, self.ctl, first_data)
        self.stream = O.svb_compress(self.read, 4, False)
        assert self.stream[: self.K].tobytes() == self.ctl.tobytes(), name
        assert first_data is None or self.stream[self.K] == first_data, name


OPTS32 = (False, 4, 1, 0)


def frames_of(build, reads, opts, **knobs):
    """the library's frames of host reads under a build's context"""
    c = T.codec(**dict(BUILDS[build], **knobs))
    comp, coff, res = T.compress(c, reads, _lib.CompressionOptions(*opts))
    host = comp.cpu().numpy()
    return [host[o : o + int(r)].copy() for o, r in zip(coff.tolist(), T.u32(res))]


def per_block(blocks, seqs):
    out, at = [], 0
    for b in blocks:
        out.append((b, seqs[at : at + int(b["nseq"])]))
        at += int(b["nseq"])
    assert at == len(seqs)
    return out


def listing(frame, stream):
    """the frame's blocks with their sequences, after libzstd has decoded it to the stream; the blocks tile the content and every
    sequence stands where its predecessors end"""
    back = O.zstd_decompress(frame, len(stream))
    assert back is not None and back.tobytes() == stream.tobytes(), "libzstd does not decode the frame to its stream"
    got = O.zstd_sequences(frame)
    assert got is not None, "the restated decoder refuses the frame"
    per = per_block(*got)
    pos = 0
    for b, sq in per:
        assert int(b["begin"]) == pos
        for s in sq:
            assert int(s["pos"]) == pos
            pos += int(s["ll"]) + int(s["ml"])
        pos += int(b["literals"]) - int(sq["ll"].sum())
        assert int(b["end"]) == pos
    assert pos == len(stream)
    return per


def found(per, lo, hi):
    """[(begin, end, [(ll, ml, offset)], tail literals)] of the blocks with sequences inside the content range [lo, hi)"""
    out = []
    for b, sq in per:
        if len(sq) and lo <= int(b["begin"]) < hi:
            out.append((int(b["begin"]), int(b["end"]), [(int(s["ll"]), int(s["ml"]), int(s["offset"])) for s in sq], int(b["literals"]) - int(sq["ll"].sum())))
    return out


def stated(ctl, extents):
    """the same of runs_ref: every extent a block of its own, tokenised as if nothing stood in front of it"""
    out = []
    for b, e in extents:
        pairs, lits = S.runs_ref(ctl[b:e]) if e - b >= S.TOK_MIN else ([], None)
        if pairs:
            out.append((b, e, [(ll, ml, 1) for ll, ml in pairs], len(lits) - sum(ll for ll, _ in pairs)))
    return out


def extents_of(build, K):
    return S.key_spans(K) if build == "spans" else [(0, K)]   # (four-byte integers: no shared table, spans of KEYSPAN)


def expected(build, c):
    """(the tokenised bytes, what the statement finds in them): the control bytes in the build's extents -- or, of a stream below
    SPLIT_MIN, which is not cut into control and data bytes, the whole stream as one region on every build"""
    if len(c.stream) < S.SPLIT_MIN:
        return c.stream, stated(c.stream, [(0, len(c.stream))])
    return c.ctl, stated(c.ctl, extents_of(build, c.K))


def check_cases(build, cases, frames):
    bad = []
    for c, f in zip(cases, frames):
        assert not isinstance(f, int), (c.name, f)
        per = listing(f, c.stream)
        text, want = expected(build, c)
        assert any(int(b["end"]) == len(text) for b, _ in per), (c.name, "no block ends where the region ends")
        got = found(per, 0, len(text))
        if got != want:
            first = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
            g, w = (got[first] if first < len(got) else None), (want[first] if first < len(want) else None)
            diff = None
            if g and w and g[:2] == w[:2]:
                k = next((i for i, (a, b) in enumerate(zip(g[2], w[2])) if a != b), min(len(g[2]), len(w[2])))
                diff = (k, g[2][k : k + 2], w[2][k : k + 2], "tails", g[3], w[3])
            bad.append((c.name, "blocks with sequences", len(got), len(want), "first difference: block", first, (g and g[:2]), (w and w[:2]), diff))
    assert not bad, (build, len(bad), "of", len(cases), bad[:6])


# ---- a. tokeniser seams ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seam_cases():
    rng = np.random.default_rng(2024)
    cases = []
    values = (0x00, 0x55, 0xFF)

    def add(name, K, runs, first_data=None):
        x = noise(rng, K)
        for s, r, v in runs:
            put_run(x, s, r, v)
        cases.append(Case(name, rng, x, first_data))

    # both sides of the first two trip seams (960, 1 920), every phase of the 16-byte cell, the lengths around the minimum and a long one
    # (and one run of 30 far from any seam: the cases with runs of RMIN - 1, where nothing is to be found at the seams, have a sequence too)
    for r in (RMIN - 1, RMIN, RMIN + 1, 40):
        for i in range(49):
            add("run %d at %d and %d" % (r, 936 + i, 1896 + i), 2100 + 7 * i, [(200, 30, 0x11), (936 + i, r, values[i % 3]), (1896 + i, r, values[(i + 1) % 3])])
    for end in (959, 960, 961):
        for r in (RMIN, 20):
            add("run %d ending at %d" % (r, end), 1500, [(end - r + 1, r, values[end % 3])])
    # back-to-back runs of different non-zero values: an end every RMIN positions, two of them in one cell; one chain across a trip seam
    for start, n in ((100, 10), (900, 12), (1, 5), (1850, 14)):
        add("chain of %d from %d" % (n, start), 2304, [(start + RMIN * j, RMIN, 1 + (j % 200)) for j in range(n)])
    add("chain of runs of RMIN + 1", 1200, [(940 + (RMIN + 1) * j, RMIN + 1, 3 + j) for j in range(6)])
    for r in (RMIN - 1, RMIN, 40):
        add("run %d from position 0" % r, 700, [(0, r, values[r % 3]), (300, 20, 0x22)])
    # a run to the region's last byte, the data bytes beginning with the same byte: the match stops at K
    for K, v in ((1024, 0x00), (1000, 0x55), (977, 0xFF), (960, 0x00), (961, 0x55), (1921, 0x00)):
        add("run to K - 1 = %d of %#x, data begins alike" % (K - 1, v), K, [(K - 30, 30, v)], first_data=v)
        add("run of RMIN to K - 1 = %d of %#x, data begins alike" % (K - 1, v), K, [(K - RMIN, RMIN, v)], first_data=v)
    add("run of RMIN - 1 to K - 1, data begins alike: no match across K", 800, [(100, 20, 0), (800 - (RMIN - 1), RMIN - 1, 0x55)], first_data=0x55)
    for K in (256, 257, 271, 300, 1000):
        add("K = %d" % K, K, [(K // 2, 25, 0), (K - 14, 14, 0x55)])
        add("K = %d, a run of 0 from 0 to K - 1 (a stream below SPLIT_MIN: one region)" % K, K, [(0, K, 0)], first_data=7)
        add("K = %d, a run of 0x55 from 0 to K - 1" % K, K, [(0, K, 0x55)], first_data=7)
    add("one run covers the region", 2048, [(0, 2048, 0)], first_data=0)
    add("K = BLOCK_MAX, one run of BLOCK_MAX - 1", BLOCK_MAX, [(1, BLOCK_MAX - 1, 0)], first_data=0)
    # on the reference alone: every case has a sequence, and the lengths around the minimum are what they were built to be
    for c in cases[: 4 * 49]:
        r = int(c.name.split()[1])
        assert sorted(ml for _, ml in S.runs_ref(c.ctl)[0]) == sorted([29] + ([r - 1, r - 1] if r >= RMIN else [])), c.name
    return cases


@functools.lru_cache(maxsize=None)
def seam_frames(build):
    return frames_of(build, [c.read for c in seam_cases()], OPTS32)


def test_reference_cases_have_sequences():
    """on the statement alone: every case of a, b and c holds at least one sequence, and every control-byte region is 256 ... BLOCK_MAX
    bytes -- so a frame without sequences is never what the statement asks for"""
    for c in seam_cases() + boundary_cases() + count_cases():
        assert S.TOK_MIN <= c.K <= BLOCK_MAX, (c.name, c.K)
        assert S.runs_ref(c.ctl)[0], c.name
        assert all(expected(b, c)[1] for b in BUILDS), c.name


@pytest.mark.parametrize("build", list(BUILDS))
def test_tokeniser_seams(build):
    cases = seam_cases()
    check_cases(build, cases, seam_frames(build))


def test_zstd_stage_alone_writes_no_sequences():
    """why the cases above are reads: the zstd stage called on its own (the caller's arena: no slot to rewrite) leaves the same control
    bytes, runs and all, without a single sequence"""
    import gpu_util as G

    cases = seam_cases()[:: 40]
    frames = G.zstd_compress([c.stream for c in cases], key_bytes=[c.K for c in cases])
    for c, f in zip(cases, frames):
        assert not isinstance(f, int), (c.name, f)
        assert all(len(sq) == 0 for _, sq in listing(f, c.stream)), c.name


@pytest.mark.parametrize("build", list(BUILDS))
def test_region_below_256_bytes_has_no_sequences(build):
    """K = 255: the region is not tokenised (S >= 256), whatever runs it holds"""
    rng = np.random.default_rng(5)
    c = Case("K = 255", rng, put_run(put_run(noise(rng, 255), 40, 60, 0), 200, 55, 0x55), first_data=0x55)
    assert S.runs_ref(c.ctl)[0]
    per = listing(frames_of(build, [c.read], OPTS32)[0], c.stream)
    assert found(per, 0, c.K) == []


# ---- b. code boundaries of the sequences section -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def boundary_cases():
    rng = np.random.default_rng(77)
    mls = sorted({v for b in ML_BASE if b >= RMIN - 1 for v in (b - 1, b) if v >= RMIN - 1})   # (a match of RMIN - 2 does not exist)
    lls = sorted({v for b in LL_BASE if b >= 1 for v in (b - 1, b) if v >= 1})                 # (nor a literal length of 0)
    own_ml, own_ll = [v for v in mls if v >= ML_BASE[-2] - 1], [v for v in lls if v >= LL_BASE[-2] - 1]
    pairs = [(1 + k % 3, ml) for k, ml in enumerate(v for v in mls if v not in own_ml)] + [(ll, RMIN - 1 + k % 5) for k, ll in enumerate(v for v in lls if v not in own_ll)]
    streams, cur, size = [], [], 0
    for p in pairs:   # as many streams as the block limit requires
        if size + sum(p) + 1 + 64 > BLOCK_MAX:
            streams.append(cur)
            cur, size = [], 0
        cur.append(p)
        size += sum(p) + 1
    streams.append(cur)
    # the two largest baselines of each kind: a stream of their own (one a length where two do not fit a block)
    streams += [[(2, ML_BASE[-2] - 1), (3, ML_BASE[-2])], [(2, ML_BASE[-1] - 1)], [(1, ML_BASE[-1])]]
    streams += [[(LL_BASE[-2] - 1, RMIN), (LL_BASE[-2], RMIN - 1)], [(LL_BASE[-1] - 1, RMIN - 1)], [(LL_BASE[-1], RMIN)]]
    cases = [Case("code boundaries %d" % i, rng, region_of(rng, p, 40 if sum(map(sum, p)) + len(p) >= 216 else 300)) for i, p in enumerate(streams)]
    have_ml = {ml for c in cases for _, ml in S.runs_ref(c.ctl)[0]}
    have_ll = {ll for c in cases for ll, _ in S.runs_ref(c.ctl)[0]}
    assert set(mls) <= have_ml and set(lls) <= have_ll
    return cases


@functools.lru_cache(maxsize=None)
def boundary_frames(build):
    return frames_of(build, [c.read for c in boundary_cases()], OPTS32)


@pytest.mark.parametrize("build", list(BUILDS))
def test_code_boundaries(build):
    cases, frames = boundary_cases(), boundary_frames(build)
    check_cases(build, cases, frames)
    if build in WHOLE:   # (a span is shorter than the largest codes' baselines)
        seqs = np.concatenate([O.zstd_sequences(f)[1] for f in frames])
        assert int((seqs["ml_code"] == 52).sum()) >= 1 and int((seqs["ll_code"] == 35).sum()) >= 1
        assert {int(v) for v in seqs["ml_code"]} >= set(range(ML_BASE.index(RMIN - 1), 53)) and {int(v) for v in seqs["ll_code"]} >= set(range(1, 36))


# ---- c. sequence counts --------------------------------------------------------------------------------------------------------------
COUNTS = (1, 127, 128, 2047, 2048, 2049, 4097)   # the count's one- and two-byte forms, the checkpoint spacing's first two doublings


@functools.lru_cache(maxsize=None)
def count_cases():
    rng = np.random.default_rng(99)
    return [Case("nseq = %d" % n, rng, region_of(rng, [(2, RMIN - 1)] * n, max(5, 300 - (RMIN + 2) * n))) for n in COUNTS]


@functools.lru_cache(maxsize=None)
def count_frames(build, trailers=1):
    return frames_of(build, [c.read for c in count_cases()], OPTS32, **({} if trailers else dict(VBZ_HIP_TRAILERS=0)))


@pytest.mark.parametrize("build", list(BUILDS))
def test_sequence_counts(build):
    cases, frames = count_cases(), count_frames(build)
    check_cases(build, cases, frames)
    if build in WHOLE:
        for n, c, f in zip(COUNTS, cases, frames):
            assert [len(sq) for _, sq in listing(f, c.stream)][0] == n, c.name


# The sequences section runs its two FSE state chains on all lanes: rounds of 256 sequences, four per lane, four-state warm-up walks of
# eight sequences (encode_zero_run_sequences).  N sequences, N around every boundary of that scheme, with literal-length and match-length
# codes of one, two, three and four table cells -- the counts and styles of test_gpu_parity.py's
# test_sequences_section_round_and_lane_boundaries, here on the path that writes a sequences section, and compared sequence by sequence.
ROUNDS = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 259, 260, 261, 511, 512, 513, 767, 768, 769, 1500, 4000)


@functools.lru_cache(maxsize=None)
def round_cases():
    rng = np.random.default_rng(11)
    cases = []
    for n in ROUNDS:
        room = (BLOCK_MAX - 400) // n   # bytes a sequence may take at the most: the region stays within a block
        ll_hi = max(2, min(40, room // 3))
        ml_hi = min(299, room - ll_hi)
        for style in range(3):
            if style == 0:      # long literal gaps (many-cell literal-length codes), matches of every length
                pairs = [(int(rng.integers(1, ll_hi + 1)), int(rng.integers(RMIN - 1, ml_hi + 1))) for _ in range(n)]
            elif style == 1:    # the shortest matches (a match-length code with two cells), one to three literals
                pairs = [(int(rng.integers(1, 4)), int(rng.integers(RMIN - 1, RMIN + 2))) for _ in range(n)]
            else:               # literal lengths 1 ... 4 and the match lengths around the minimum: the codes with several cells
                pairs = [(int(rng.integers(1, 5)), RMIN - 1 + int(rng.integers(0, 2)) * int(rng.integers(0, min(40, ml_hi - RMIN + 2)))) for _ in range(n)]
            cases.append(Case("%d sequences, style %d" % (n, style), rng, region_of(rng, pairs, 300)))
    return cases


@functools.lru_cache(maxsize=None)
def round_frames(build):
    return frames_of(build, [c.read for c in round_cases()], OPTS32)


@pytest.mark.parametrize("build", list(BUILDS))
def test_sequence_rounds_and_lanes(build):
    cases, frames = round_cases(), round_frames(build)
    assert all(S.TOK_MIN <= c.K <= BLOCK_MAX and len(c.stream) >= S.SPLIT_MIN and S.runs_ref(c.ctl)[0] for c in cases)
    check_cases(build, cases, frames)


# ---- d. checkpoints ----------------------------------------------------------------------------------------------------------------------
def trailer_of(frame):
    """(spacing, words) of the frame's checkpoint trailer, or None"""
    t = E.frame_trailers(frame).get(CP_MAGIC)
    if t is None:
        return None
    head = int.from_bytes(t[:4], "little")
    spacing, count = head & 0xFFFF, head >> 16
    assert len(t) == 4 + 4 * count + 4 and int.from_bytes(t[-4:], "little") == len(t) + 8, (len(t), count)
    return spacing, [int.from_bytes(t[4 + 4 * j : 8 + 4 * j], "little") for j in range(count)]


@pytest.mark.parametrize("build", WHOLE)
def test_checkpoints(build):
    """every frame of a, b and c: spacing, count and every word of the trailer are the statement's for the listing of the frame's block
    of zero-run sequences; a block of up to CP_MIN_SPACING sequences has no checkpoint and the frame no trailer"""
    bad, with_trailer, spacings = [], 0, set()
    for cases, frames in ((seam_cases(), seam_frames(build)), (boundary_cases(), boundary_frames(build)), (count_cases(), count_frames(build)),
                          (round_cases(), round_frames(build))):
        for c, f in zip(cases, frames):
            sq = [q for _, q in listing(f, c.stream) if len(q)]
            assert len(sq) <= 1, c.name
            spacing, words = S.checkpoints_ref(sq[0]) if sq else (S.CP_MIN_SPACING, [])
            got, want = trailer_of(f), ((spacing, words) if words else None)
            if got != want:
                k = next((j for j, (a, b) in enumerate(zip(got[1], want[1])) if a != b), None) if got and want else None
                bad.append((c.name, got and (got[0], len(got[1])), want and (want[0], len(want[1])), "first differing word", k,
                            None if k is None else (hex(got[1][k]), hex(want[1][k]))))
            with_trailer += want is not None
            spacings.add(spacing)
    assert not bad, (build, len(bad), bad[:6])
    assert with_trailer >= 6 and spacings >= {32, 64, 128}


def test_no_trailers_on_request():
    cases, frames, plain = count_cases(), count_frames("staged"), count_frames("staged", trailers=0)
    for c, f, p in zip(cases, frames, plain):
        assert trailer_of(p) is None and E.frame_trailers(p) == {}, c.name
        assert p.tobytes() == f[: len(p)].tobytes(), c.name   # (the frame in front of the trailer is the same)
    assert any(trailer_of(f) is not None for f in frames)


# ---- e. the long-repeat matcher --------------------------------------------------------------------------------------------------------
def template_read(rng, period, total, changed=0):
    """a template of `period` samples tiled to `total`; its deltas take one byte (|d| <= 50) or two (300 <= |d| <= 400), and `changed`: every
    that many samples one is raised by 1 -- which changes two deltas by 1 and no delta's byte count"""
    d = rng.integers(-50, 51, period)
    big = rng.permutation(period)[: period // 9]
    d[big] = np.where(np.arange(len(big)) & 1, -1, 1) * rng.integers(300, 401, len(big))
    t = 1000 + np.cumsum(d)
    x = np.tile(t, total // period + 1)[:total]
    if changed:
        x[changed::changed] += 1
    assert x.min() > -32000 and x.max() < 32000
    return x.astype(np.int16)


def implied_distance(stream, K, first, count):
    """data bytes of the values first ... first + count - 1, from the control bytes"""
    codes = ((stream[:K, None] >> np.array([0, 2, 4, 6], np.uint8)) & 3).reshape(-1)
    return int((codes[first : first + count] + 1).sum())


@functools.lru_cache(maxsize=None)
def matcher_reads():
    """[(name, read, options, stream, K, implied distance of the data bytes)]"""
    rng = np.random.default_rng(31)
    out = []
    for total in (70001, 150000):
        for changed in (0, 977):
            x = template_read(rng, 7001, total, changed)
            st = O.svb_compress(x, 2, True, 1)
            K = (total + 3) // 4
            out.append(("template 7001 x %d%s" % (total, ", every 977th changed" if changed else ""), x, (True, 2, 1, 1), st, K, implied_distance(st, K, 7001, 7001)))
    x = np.arange(600000).astype(np.int8)
    st = O.svb_compress(x, 1, True, 0)
    out.append(("int8 iota of 600000", x, (True, 1, 1, 0), st, 150000, implied_distance(st, 150000, 256, 256)))
    return out


def test_matcher_sequences():
    reads = matcher_reads()
    f16 = frames_of("staged", [r[1] for r in reads[:4]], reads[0][2])
    f8 = frames_of("staged", [reads[4][1]], reads[4][2])
    for (name, x, opts, stream, K, D), f in zip(reads, f16 + f8):
        per = listing(f, stream)
        assert any(int(b["end"]) == K for b, _ in per), (name, "no block ends where the control bytes end")
        regions = {"control": (0, K), "data": (K, len(stream))}
        explicit = {"control": set(), "data": set()}
        for b, sq in per:
            which = "control" if int(b["begin"]) < K else "data"
            r0, r1 = regions[which]
            begin, end = int(b["begin"]), int(b["end"])
            assert r0 <= begin and end <= r1, (name, begin, end, K)
            if len(sq) == 0:
                continue
            offs = {int(v) for v in sq["offset"]}
            assert len(offs) == 1, (name, begin, "offsets", sorted(offs)[:4])
            off = offs.pop()
            assert (begin - r0) % 16 == 0 and end - begin <= BLOCK_MAX, (name, which, begin - r0, end - begin)
            got = [(int(s["ll"]), int(s["ml"])) for s in sq]
            tail = int(b["literals"]) - int(sq["ll"].sum())
            if (sq["ofv"] > 3).all():      # the matcher: explicit offsets
                explicit[which].add(off)
                pairs, lits = S.period_ref(stream[r0:r1], begin - r0, end - r0, off)
            else:                          # zero runs: the repeat offset, 1
                assert (sq["ofv"] == 1).all() and off == 1, (name, begin)
                pairs, lits = S.runs_ref(stream[begin:end])
            k = next((i for i, (a, c) in enumerate(zip(got, pairs)) if a != c), None)
            assert got == pairs and tail == len(lits) - sum(ll for ll, _ in pairs), (name, which, begin, end, off, len(got), len(pairs), k,
                                                                                      None if k is None else (got[k], pairs[k]), tail)
        # the data bytes: the distance the read's construction implies, and no block of them left without its matches
        assert explicit["data"] == {D}, (name, explicit, D)
        assert len(explicit["control"]) <= 1 and all(d >= 64 for d in explicit["control"]), (name, explicit)
        for b, sq in per:
            begin, end = int(b["begin"]), int(b["end"])
            if len(sq) == 0 and begin >= K:
                assert S.period_ref(stream[K:], begin - K, end - K, D)[0] == [], (name, "a block of data bytes without sequences", begin, end)
            if len(sq) == 0 and begin < K and explicit["control"]:
                Dk = next(iter(explicit["control"]))
                assert S.period_ref(stream[:K], begin, end, Dk)[0] == [], (name, "a block of control bytes without sequences", begin, end)
        if K > BLOCK_MAX and not explicit["control"]:   # control bytes beyond a block: zero-run sequences per chunk
            assert found(per, 0, K), (name, "no zero-run sequences in the control bytes")
