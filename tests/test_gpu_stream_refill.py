"""The stream decoder's shared refill (zstd_decode_fast.hip: fast_streams_kernel, VBZ_FS_TRIGGER) on the frames in which a refill that
the 64 lanes of a wavefront make TOGETHER can go wrong and one that every lane makes for itself cannot (-m gpu).

With a trigger a lane that has room is not refilled until some lane of its wavefront is low, and a lane that is low makes every lane
with room refill.  So the cases are frames whose lanes disagree: streams of the table's longest codes beside streams of its shortest
(the fast lanes must trigger refills the slow ones never have room for, and must not run dry; the slow ones must keep their data through
many refused refills); every phase of the first 64-byte line; streams that end in the head or the tail code; idle lanes; lanes that
finish many bursts before the others; two tables.

Every case is a batch of at most 64 contents that the library's zstd stage compresses, the library decodes -- decode_paths() must say that
the batched own-frame decoder took EVERY frame: a frame it leaves to the one-wavefront decoder proves nothing here -- and the oracle decodes
(oracle_lib.zstd_decompress: libzstd); the three must agree byte for byte.  The shape a case claims (stream sizes, code lengths per symbol,
streams per frame) is read back from the frames themselves (stream_sizes) and asserted.

How the encoder cuts a content of N bytes (zstd_encode.hip): a region (the whole content, or with key_bytes = K the first K bytes and the
rest) is nblk = ceil(S / T) blocks of S / nblk bytes, T = max(4096, ceil(N / 14)); a block is four streams of ceil(bytes / 4) symbols (the
last one the rest); a region has one table, built from its exact histogram below 32 KB or 240 distinct values.  Runs of 12 equal bytes and
more are kept out of every content (the tokeniser would turn them into sequences)."""
import functools

import numpy as np
import pytest

import gpu_util as G
import oracle_lib as O
from huffman_corpus import RMIN, fib, longest_run

pytestmark = pytest.mark.gpu

LINE = 64            # bytes of one request of the stream decoder
PERIOD_WORST = 22    # bytes 16 symbols of 11 bits take: a stream shorter than this ends inside its first period whatever its codes


# ---- reading a frame back -----------------------------------------------------------------------------------------------------------
def stream_sizes(frame):
    """[(symbols, bytes, has a tree)] for the Huffman streams of the frame's blocks, in frame order (RFC 8878 3.1.1.3.1); a block whose
    literals are not four Huffman streams raises"""
    f = bytes(frame)
    pos = O.zstd_frame_geometry(frame)[0]
    out = []
    while True:
        bh = int.from_bytes(f[pos : pos + 3], "little")
        last, btype, bsize = bh & 1, (bh >> 1) & 3, bh >> 3
        assert btype == 2, "not a compressed block"
        p = pos + 3
        ltype, fmt = f[p] & 3, (f[p] >> 2) & 3
        assert ltype in (2, 3) and fmt != 0, "literals not in four Huffman streams"
        hlen, bits = {1: (3, 10), 2: (4, 14), 3: (5, 18)}[fmt]
        v = int.from_bytes(f[p : p + hlen], "little")
        regen, comp = (v >> 4) & ((1 << bits) - 1), (v >> (4 + bits)) & ((1 << bits) - 1)
        p += hlen
        tree = 0
        if ltype == 2:
            hb = f[p]
            tree = 1 + hb if hb < 128 else 1 + (hb - 127 + 1) // 2
        j = p + tree
        s = [int.from_bytes(f[j + 2 * k : j + 2 * k + 2], "little") for k in range(3)]
        s.append(comp - tree - 6 - sum(s))
        q = (regen + 3) // 4
        out += [(n, b, ltype == 2) for n, b in zip([q, q, q, regen - 3 * q], s)]
        pos += 3 + bsize
        if last:
            return out


def roundtrip(contents, key_bytes=None, skew=0, frames=None):
    """compress (unless `frames` are given), decode with the frames at source offsets = skew mod 64, compare with the oracle's decode and
    the contents; every frame must have gone to the batched own-frame decoder.  Returns the frames."""
    if frames is None:
        frames = G.zstd_compress(contents, key_bytes)
        bad = [(i, f) for i, f in enumerate(frames) if isinstance(f, int)]
        assert not bad, bad
    old = G.SRC_SKEW
    G.SRC_SKEW = skew
    try:
        back = G.zstd_decompress(frames, [c.nbytes for c in contents])
        paths = G.codec().decode_paths()
    finally:
        G.SRC_SKEW = old
    assert paths[0] == len(contents) and paths[1] == len(contents), "frames left to the one-wavefront decoder: %r" % (paths,)
    for i, (c, f, g) in enumerate(zip(contents, frames, back)):
        want = O.zstd_decompress(f, c.nbytes)
        assert want is not None, "the oracle refuses frame %d" % i
        assert not isinstance(g, int), (i, hex(g))
        assert g.tobytes() == want.tobytes(), "frame %d: not the oracle's bytes" % i
        assert want.tobytes() == c.tobytes(), "frame %d: not the content" % i
    return frames


def no_runs(make, seed):
    """make(rng) -> bytes, re-drawn until it has no run of RMIN equal bytes"""
    for attempt in range(64):
        a = make(np.random.default_rng([seed, attempt]))
        if longest_run(a) < RMIN:
            return a
    raise AssertionError("no arrangement without a run of %d" % RMIN)


def skewed(rng, n, probs, first=1):
    """n bytes over the values first, first + 1, ... drawn with the given probabilities"""
    p = np.asarray(probs, np.float64)
    return (first + rng.choice(len(p), n, p=p / p.sum())).astype(np.uint8)


# ---- extreme rates in one frame -----------------------------------------------------------------------------------------------------
# 56 streams of 1 024 symbols (14 blocks of 4 096 bytes) under ONE table with 1-bit to 11-bit codes.  The head of the histogram is the
# Fibonacci comb of huffman_corpus (fib(9) descending on the values 1 .. 9, scaled): codes of 1, 2, 3 ... bits.  The Fibonacci counts for
# the 11-bit limit themselves (fib(21)) put 143 of 28 656 bytes on the 11-bit codes, not one stream's worth; so the comb's tail is widened
# to 192 values (64 .. 255) of 32 bytes each, 2^-10.8 of the content: 11 bits, and six whole streams of nothing else.
STREAM = 1024
N_EXTREME = 14 * 4 * STREAM
FAST = (4, 13, 22, 31, 40, 49)     # streams of 11-bit codes only
N_SLOW = 20                        # streams of the two shortest codes only


def extreme_content(seed, fast=FAST, n_slow=N_SLOW):
    """(content, fast stream indices, slow stream indices)"""
    rng = np.random.default_rng(seed)
    nstreams = N_EXTREME // STREAM
    tail_total = len(fast) * STREAM
    assert tail_total % 192 == 0
    head = np.array(fib(9)[::-1], np.int64)
    k = (N_EXTREME - tail_total) // head.sum()
    head = head * k
    head[0] += N_EXTREME - tail_total - head.sum()
    rest = [j for j in range(nstreams) if j not in fast]
    slow = rest[0::2][:n_slow]
    mixed = [j for j in rest if j not in slow]
    streams = {}
    tail = rng.permutation(np.repeat(np.arange(64, 256, dtype=np.uint8), tail_total // 192))
    for i, j in enumerate(fast):
        streams[j] = tail[i * STREAM : (i + 1) * STREAM]
    unit = np.array([1] * 7 + [2], np.uint8)   # seven of the shortest code, one of the next: no run of 12
    for j in slow:
        streams[j] = np.roll(np.tile(unit, STREAM // 8), int(rng.integers(0, 8)))
    head[0] -= n_slow * STREAM * 7 // 8
    head[1] -= n_slow * STREAM // 8
    assert head.min() > 0 and head.sum() == len(mixed) * STREAM
    pool = no_runs(lambda r: r.permutation(np.repeat(np.arange(1, 10, dtype=np.uint8), head)), seed)
    for i, j in enumerate(mixed):
        streams[j] = pool[i * STREAM : (i + 1) * STREAM]
    content = np.concatenate([streams[j] for j in range(nstreams)])
    assert longest_run(content) < RMIN and len(content) == N_EXTREME
    return content, list(fast), slow


def check_extreme(frame, fast, slow, first_stream=0):
    """the streams of 11-bit codes take at least 10 bits a symbol, those of the shortest codes at most 2"""
    S = stream_sizes(frame)[first_stream:]
    assert len(S) == N_EXTREME // STREAM and all(n == STREAM for n, _, _ in S), [n for n, _, _ in S]
    assert all(8 * S[j][1] >= 10 * STREAM for j in fast), [S[j] for j in fast]
    assert all(8 * S[j][1] <= 2 * STREAM + 16 for j in slow), [S[j] for j in slow]


def test_extreme_rates_in_one_frame():
    """Six lanes at 11 bits a symbol (a 64-byte line lasts them 47 symbols: they trigger in every third period), twenty at 1.1 bits (a line
    lasts them 450 symbols: they are refused hundreds of times with a full ring) and thirty in between, in one wavefront; the fast streams
    in other lanes from frame to frame."""
    cases = [extreme_content(11 + k, fast=tuple((j + 3 * k) % 56 for j in FAST)) for k in range(8)]
    frames = roundtrip([c for c, _, _ in cases])
    for f, (_, fast, slow) in zip(frames, cases):
        check_extreme(f, fast, slow)


# ---- every phase of the first line ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def line_contents():
    """64 contents of one block: 56 whose four streams are about one 64-byte line long (133 .. 147 symbols at ~ 3.7 bits), 8 whose
    streams are shorter than one period's worst case (65 .. 74 symbols of two values, a bit each: the encoder writes a content below
    256 bytes as ONE stream, which the batched decoder leaves to the one-wavefront decoder, so a stream has at least 64 symbols)"""
    out = []
    geo = 0.8 ** np.arange(24)
    for k in range(56):
        out.append(no_runs(lambda r: skewed(r, 532 + k, geo), 100 + k))
    for k in range(8):
        out.append(no_runs(lambda r: skewed(r, 260 + 5 * k, [0.5, 0.5]), 200 + k))
    return out


@functools.lru_cache(maxsize=1)
def line_frames():
    contents = line_contents()
    frames = roundtrip(contents)
    sizes = sorted(b for f in frames for _, b, _ in stream_sizes(f))
    for want in (LINE - 1, LINE, LINE + 1):
        assert want in sizes, "no stream of %d bytes" % want
    assert sum(1 for b in sizes if b < PERIOD_WORST) >= 16, "too few streams below one period's worst case"
    return frames


@pytest.mark.parametrize("k", [0, 1, 15, 16, 63])
def test_every_phase_of_the_first_line(k):
    """The frames at source offsets = k mod 64: with the streams' own offsets in their frames the bytes between a stream's end and the top
    of its first line take every value 0 .. 63.  Among the streams are some of exactly one line, of one line less and more a byte, and
    some shorter than the worst case of one period (22 bytes), whose only line is the first."""
    roundtrip(line_contents(), skew=k, frames=line_frames())


# ---- only head and tail code -----------------------------------------------------------------------------------------------------------
# (The issue's "fewer than 16 symbols" does not exist on this path: below 256 bytes the encoder writes a content as ONE Huffman stream,
# and the scan leaves such a frame to the one-wavefront decoder -- measured on the parent library: contents of 65 .. 163 bytes all went
# there.  The shortest streams the batched decoder meets are the 62 .. 65 symbols here: the head, a few groups, the tail.)
HEAD_TAIL_N = [256, 257, 258, 259,       # 64 / 65 symbols a stream, the last one 64, 62, 63, 64: the shortest four-stream contents
               4 * 77, 4 * 100 + 2, 4 * 111 + 1, 4 * 127,   # inside the groups
               4 * 128, 4 * 129, 4 * 143, 4 * 144, 4 * 145,   # one burst, and 1, 15, 16, 17 symbols
               4 * 129 - 3, 4 * 144 - 2, 4 * 145 - 1]         # ... with a last stream of another length


def test_only_head_and_tail_code():
    """Streams of 62 .. 65 symbols, of 77 .. 127, of exactly 128 and of 128 + 1, 15, 16, 17: the burst loop runs once or not at all, and
    every look at the ring is made by the head and tail code (symbols one at a time, groups of 16).  Four contents per length: the
    streams' output offsets, which decide how many symbols the head takes, differ from stream to stream."""
    probs = [0.4, 0.25, 0.15, 0.1, 0.06, 0.04]
    contents = [no_runs(lambda r: skewed(r, n, probs), 300 + 10 * i + s) for i, n in enumerate(HEAD_TAIL_N) for s in range(4)]
    assert len(contents) == 64
    frames = roundtrip(contents)
    counts = {n for f in frames for n, _, _ in stream_sizes(f)}
    for want in (62, 63, 64, 65, 77, 127, 128, 129, 143, 144, 145):
        assert want in counts, want


# ---- fewer than 64 streams, finished lanes, two tables -------------------------------------------------------------------------------
def test_fewer_than_64_streams():
    """Frames of 4, 8, 12, 20 and 40 streams whose lanes run at mixed rates: the idle lanes of the wavefront neither trigger nor block."""
    geo = 0.7 ** np.arange(40)
    contents, want = [], []
    for i, (n, streams) in enumerate(((3001, 4), (5000, 8), (9001, 12), (20000, 20), (40001, 40))):
        for s in range(4):
            contents.append(no_runs(lambda r: skewed(r, n, geo), 400 + 10 * i + s))
            want.append(streams)
    frames = roundtrip(contents)
    assert [len(stream_sizes(f)) for f in frames] == want


def two_region_content(seed, short_first):
    """(content, key_bytes, fast, slow).  short_first: 600 bytes of six values (a table of short codes, four streams of 150 symbols that
    finish seven bursts before the others) in front of the 56 extreme streams (the 11-bit table: the SECOND table is the wide one).
    Otherwise the extreme streams first and 2 400 bytes of six values behind them (four streams of 600 symbols)."""
    body, fast, slow = extreme_content(seed)
    probs = [0.4, 0.25, 0.15, 0.1, 0.06, 0.04]
    if short_first:
        few = no_runs(lambda r: skewed(r, 600, probs, first=20), seed + 1000)
        return np.concatenate([few, body]), len(few), fast, slow
    few = no_runs(lambda r: skewed(r, 2400, probs, first=20), seed + 2000)
    return np.concatenate([body, few]), len(body), fast, slow


def test_two_tables_and_finished_lanes():
    """Sixty streams under two tables: four short streams under a table of six values and the 56 extreme streams under the 11-bit table.
    With the short region first the second table is the wide one (tlog1 > tlog0: it takes the large slot) and lanes 0 .. 3 finish seven
    bursts before the others; with the short region last the first table is the wide one and lanes 56 .. 59 finish three bursts early.
    A finished lane must not hold the trigger open, and its ring is no longer anybody's business."""
    cases = [two_region_content(500 + k, short_first=k % 2 == 0) for k in range(8)]
    contents = [c for c, _, _, _ in cases]
    # (N is 57 944 or 59 744, so T = ceil(N / 14) is 4 139 or 4 268: the 57 344 extreme bytes are still 14 blocks of 4 096)
    frames = roundtrip(contents, key_bytes=[k for _, k, _, _ in cases])
    for i, (f, (c, k, fast, slow)) in enumerate(zip(frames, cases)):
        S = stream_sizes(f)
        assert len(S) == 60 and sum(1 for _, _, tree in S if tree) == 8, (i, len(S))   # two blocks that bring a tree, four streams each
        short = S[:4] if i % 2 == 0 else S[-4:]
        assert all(n in (150, 600) and 8 * b <= 5 * n for n, b, _ in short), short    # six values: no code above five bits
        check_extreme_streams = S[4:] if i % 2 == 0 else S[:-4]
        assert all(8 * check_extreme_streams[j][1] >= 10 * check_extreme_streams[j][0] for j in fast), i
        assert all(8 * check_extreme_streams[j][1] <= 2 * check_extreme_streams[j][0] + 16 for j in slow), i
