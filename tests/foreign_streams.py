"""svb streams another writer could hand to the typed decode calls, and the numpy statement of what the int16 zig-zag decoder makes of
them (svb_kernels.hip: svb_decode_range, I16DecPairs::run).  This library and the oracle write codes 0 and 1 only (one- and two-byte
values); a foreign stream may hold codes 2 and 3, may be shorter than it announces, and may put more bytes into a pair of tiles than a
stage buffer holds -- each of which ends the decoder's pair loop and hands the read over to its tile loop.  decode() states the
reference's values for any codes (its SIMD body keeps 16 bits of a wide code, its scalar tail all of them), pair_exit() states where the
pair loop stops and why, catalogue() is the list of streams the sinks of svb_store.h are held to by tests/test_gpu_foreign_streams.py.
tests/test_foreign_streams_ref.py holds decode() to the oracle and the catalogue to the conditions the device tests rely on.  A plain
module, no GPU."""
import collections
import os
import re

import numpy as np

import oracle_lib as O

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vbz_compression_amd", "csrc")


def _arith(text, names):
    """the value of a constant expression of integers, names, + - * / and brackets (C's integer division)"""
    for k, v in names.items():
        text = re.sub(r"\b%s\b" % k, str(v), text)
    assert re.fullmatch(r"[\d\s+\-*/()]+", text), text
    return int(eval(text.replace("/", "//"), {"__builtins__": {}}))   # (digits and operators only, by the line above)


def _constants():
    with open(os.path.join(CSRC, "svb_store.h")) as f:
        wg = int(re.search(r"constexpr int WG = (\d+);", f.read()).group(1))
    with open(os.path.join(CSRC, "svb_kernels.hip")) as f:
        src = f.read()
    pairs = src[src.index("struct I16DecPairs") :]
    buf = _arith(re.search(r"\bBUF = ([^;,]+)[;,]", pairs).group(1), {"WG": wg})
    seg_tiles = int(re.search(r"constexpr int SEG_TILES = (\d+);", src).group(1))
    return wg, buf, seg_tiles


WG, BUF, SEG_TILES = _constants()
T = WG * 8            # a tile: eight values per thread
P = 2 * T             # a pair of tiles: one trip of the pair loop
SEG = T * SEG_TILES   # a segment of the large-read path
assert (T, P, SEG) == (2048, 4096, 16384), (T, P, SEG)

WIDE, SHORT, OVER = "wide code", "stream shorter than announced", "more bytes than a stage buffer"
Row = collections.namedtuple("Row", "name stream n tags")


# ---- the statement ----------------------------------------------------------------------------------------------------------------------
def layout(stream, n):
    """(codes, data offset of every value, announced data bytes, data bytes present) of a stream of n values"""
    stream = np.asarray(stream, np.uint8)
    K = (n + 3) // 4
    assert len(stream) >= K, (len(stream), K)
    codes = ((stream[:K, None] >> np.array([0, 2, 4, 6], np.uint8)) & 3).reshape(-1)[:n].astype(np.int64)
    ends = np.cumsum(codes + 1)
    return codes, ends - (codes + 1), int(ends[-1]) if n else 0, len(stream) - K


def decode(stream, n, body=None):
    """(int16 values, body mask) the reference's int16 zig-zag decoder gives for n values of `stream`, whatever its codes; None where
    the bytes its control bytes announce are not the bytes present.  Value i is masked to 16 bits iff it lies in the SIMD body: its
    group of eight is a whole one in front of the last, (i >> 3) < (n >> 3), and at least 32 data bytes are left where the group begins.
    body: another mask than the reference's (True: the mask on everywhere)"""
    stream = np.asarray(stream, np.uint8)
    codes, off, announced, present = layout(stream, n)
    if announced != present:
        return None
    K = (n + 3) // 4
    data = np.concatenate([stream[K:], np.zeros(4, np.uint8)]).astype(np.uint64)
    v = np.zeros(n, np.uint64)
    for j in range(4):
        v |= np.where(codes >= j, data[off + j] << np.uint64(8 * j), np.uint64(0))
    i = np.arange(n)
    mask = ((i >> 3) < (n >> 3)) & (present - off[(i >> 3) << 3] >= 32)
    if body is not None:
        mask = np.broadcast_to(np.asarray(body, bool), (n,)).copy()
    v = np.where(mask, v & np.uint64(0xFFFF), v)
    d = (v >> np.uint64(1)) ^ (np.uint64(0) - (v & np.uint64(1)))
    return (np.cumsum(d, dtype=np.uint64) & np.uint64(0xFFFF)).astype(np.uint16).view(np.int16), mask


def pair_exit(stream, n, addr16, first=0, end=None):
    """(pair index, reason) where I16DecPairs::run, started at value `first` of a range that ends at `end`, stops in front of a pair and
    hands over to the tile loop; None where it decodes every whole pair of the range.  addr16: the device address of the stream's first
    byte mod 16 (a pair's bytes are staged from the 16-byte line its first byte lies in, so `mis` bytes of the buffer go to alignment)"""
    end = n if end is None else end
    codes, off, _, present = layout(stream, n)
    K = (n + 3) // 4
    pos = int(off[first]) if first < n else 0
    pair = 0
    while end - first >= 2 * T:
        c = codes[first : first + P]
        size = int((c + 1).sum())
        mis = (addr16 + K + pos) % 16
        if (c >= 2).any():
            return pair, WIDE
        if pos + size > present:
            return pair, SHORT
        if mis + size + 16 > BUF:
            return pair, OVER
        pos += size
        first += P
        pair += 1
    return None


# ---- reads ------------------------------------------------------------------------------------------------------------------------------
def quiet(rng, n, bound=3000):
    """a bounded walk, steps inside +-40: one-byte codes throughout"""
    c = np.cumsum(rng.integers(-40, 41, n))
    return (np.abs((c + bound) % (4 * bound) - 2 * bound) - bound).astype(np.int16)   # (folded back at +-bound: a step keeps its size)


def noise(rng, n):
    """the whole int16 range: two-byte codes but for one value in 256"""
    return rng.integers(-32768, 32768, n).astype(np.int16)


def border(rng, n):
    """a walk whose steps lie on either side of the one-byte / two-byte border of the zig-zag code (254, 255 | 256, 257), and 0, 1, -1"""
    return np.cumsum(rng.choice(np.array([127, -128, 128, -129, 0, 1, -1]), n)).astype(np.int16)


KINDS = {"quiet": quiet, "noise": noise, "border": border}


def mix(rng, parts):
    """one read of segments (kind, samples) joined end to end"""
    return np.concatenate([KINDS[kind](rng, m) for kind, m in parts])


def compress(x):
    stream = O.svb_compress(np.ascontiguousarray(x, np.int16), 2, True)
    assert not isinstance(stream, int), hex(stream)
    assert layout(stream, len(x))[0].max(initial=0) <= 1, "the oracle wrote a wide code"
    return stream


def with_two_byte_codes(rng, n, at, count):
    """a quiet read of n samples whose values at ... at + count - 1 take two bytes (steps of +-200), every other value one"""
    d = rng.integers(-40, 41, n)
    d[at : at + count] = np.where(np.arange(count) % 2 == 0, 200, -200)
    x = np.cumsum(d)
    assert np.abs(x).max() < 30000
    return x.astype(np.int16)


# ---- edits ------------------------------------------------------------------------------------------------------------------------------
def _set_code(stream, value, code):
    out = np.array(stream, np.uint8)
    sh = 2 * (value & 3)
    out[value >> 2] = (int(out[value >> 2]) & ~(3 << sh) & 0xFF) | (code << sh)
    return out


def widen_short(stream, n, value, code):
    """the value's code set to 2 or 3, without the bytes that code announces"""
    assert code in (2, 3)
    assert layout(stream, n)[0][value] <= 1
    return _set_code(stream, value, code)


def widen(stream, n, value, code, fill):
    """the value's code set to 2 or 3 and the bytes that code announces put behind the value's own, each `fill`: >= 0x80 and odd, so bits
    8 ... 15 of a one-byte value change wherever it is kept to 16 bits, and bit 16 -- bit 15 of the delta -- is set wherever it is not"""
    assert fill >= 0x80 and fill & 1, fill
    codes, off, _, _ = layout(stream, n)
    K = (n + 3) // 4
    at = K + int(off[value]) + int(codes[value]) + 1
    out = widen_short(stream, n, value, code)
    return np.concatenate([out[:at], np.full(code - int(codes[value]), fill, np.uint8), out[at:]])


def wide_values(stream, n):
    return np.flatnonzero(layout(stream, n)[0] >= 2)


# ---- the catalogue ----------------------------------------------------------------------------------------------------------------------
N_RAGGED = 12 * T + 77
N_WHOLE = 8 * T
N_SEGS = 40_000


def catalogue(rng, addr16=0):
    """rows (name, stream, n, tags).  addr16: the alignment the two BUF-limit rows are built for (their slot's address mod 16)"""
    rows = []

    def add(name, stream, n, *tags):
        rows.append(Row(name, np.ascontiguousarray(stream, np.uint8), n, frozenset(tags)))

    ragged, whole = quiet(rng, N_RAGGED), quiet(rng, N_WHOLE)
    s_ragged, s_whole = compress(ragged), compress(whole)
    # intact
    add("quiet 12T + 77", s_ragged, N_RAGGED, "intact")
    add("quiet 8T", s_whole, N_WHOLE, "intact")
    add("border 6T + 3", compress(border(rng, 6 * T + 3)), 6 * T + 3, "intact")
    # a pair of more bytes than a stage buffer; quiet behind the noise, so the tile loop's whole-tile branch runs behind the exit (three
    # tiles of it and a ragged end -- but behind the last whole pair, where less than a pair is left by definition: one tile and the end)
    for name, parts in (("noise fills pair 0", [("noise", P), ("quiet", 3 * T + 5)]),
                        ("noise fills pair 1", [("quiet", P), ("noise", P), ("quiet", 3 * T + 9)]),
                        ("noise fills pair 3", [("quiet", 3 * P), ("noise", P), ("quiet", 3 * T + 1)]),
                        ("noise fills the last whole pair", [("quiet", 2 * P), ("noise", P), ("quiet", T + 77)]),
                        ("a pair half noise fits", [("quiet", P), ("noise", T), ("quiet", T), ("quiet", 3 * T + 13)])):
        x = mix(rng, parts)
        add(name, compress(x), len(x), "buf")
    # pair 1 of exactly BUF - 16 - mis bytes, and of one more: P one-byte values of which `two` take a second byte
    n = 2 * P + 3 * T + 21
    mis = (addr16 + (n + 3) // 4 + P) % 16   # (pair 0: P one-byte values)
    two = BUF - 16 - mis - P
    add("pair 1 at the buffer's limit", compress(with_two_byte_codes(rng, n, P + 5, two)), n, "buf", "limit", "fits")
    add("pair 1 one byte over the limit", compress(with_two_byte_codes(rng, n, P + 5, two + 1)), n, "buf", "limit", "over")
    # wide codes with their bytes
    at_ragged = [("value 0", 0), ("value 7", 7), ("value P - 1", P - 1), ("value P", P), ("value 2P + 3", 2 * P + 3),
                 ("the last whole pair", (N_RAGGED // P - 1) * P + 1001), ("the first value of the ragged tile", N_RAGGED // T * T),
                 ("value n - 40", N_RAGGED - 40), ("value n - 9", N_RAGGED - 9), ("value n - 8", N_RAGGED - 8), ("value n - 1", N_RAGGED - 1)]
    for what, value in at_ragged:
        for code in (2, 3):
            add("code %d at %s of 12T + 77" % (code, what), widen(s_ragged, N_RAGGED, value, code, 0x81 + 2 * int(rng.integers(0, 63))), N_RAGGED, "wide")
    for g, value in ((3, N_WHOLE - 24 + 5), (2, N_WHOLE - 16), (1, N_WHOLE - 1)):
        for code in (2, 3):
            add("code %d in group %d from the end of 8T" % (code, g), widen(s_whole, N_WHOLE, value, code, 0x81 + 2 * int(rng.integers(0, 63))), N_WHOLE,
                "wide", "last groups")
    # defects: the int16 decode's verdict is the oracle's VBZ_STREAMVBYTE_STREAM_ERROR
    add("code 2 at value P + 9 without its bytes", widen_short(s_ragged, N_RAGGED, P + 9, 2), N_RAGGED, "wide", "error", "without bytes")
    add("code 3 at value n - 3 without its bytes", widen_short(s_ragged, N_RAGGED, N_RAGGED - 3, 3), N_RAGGED, "wide", "error", "without bytes")
    add("quiet 8T, last byte missing", s_whole[:-1], N_WHOLE, "error", "byte missing")
    s_border = compress(border(rng, N_WHOLE))
    add("border 8T, last byte missing", s_border[:-1], N_WHOLE, "error", "byte missing")
    # random control bytes with the bytes they announce
    for n in (4096 + 8, 9000):
        add("random control bytes, %d values" % n, random_stream(rng, n), n, "random")
    # three segments of the large-read path
    x = quiet(rng, N_SEGS)
    s = compress(x)
    add("three segments, code 3 at value 20 003", widen(s, N_SEGS, 20_003, 3, 0xC3), N_SEGS, "wide", "segments")
    add("three segments, code 2 eight values before the end", widen(s, N_SEGS, N_SEGS - 8, 2, 0x9D), N_SEGS, "wide", "segments")
    burst = x.copy()
    burst[SEG - T // 2 : SEG + T // 2] = noise(rng, T)
    add("three segments, noise across the first seam", compress(burst), N_SEGS, "noise", "segments")
    add("three segments, intact", s, N_SEGS, "intact", "segments")
    assert len({r.name for r in rows}) == len(rows)
    return rows


def random_stream(rng, n):
    """random control bytes (every code) and as many random data bytes as they announce"""
    K = (n + 3) // 4
    keys = rng.integers(0, 256, K).astype(np.uint8)
    announced = layout(keys, n)[2]
    return np.concatenate([keys, rng.integers(0, 256, announced).astype(np.uint8)])
