"""A catalogue of values and streams for the generic svb workers (svb_kernels.hip: the five generic instantiations of svb_encode_range /
svb_decode_range, their segmented forms) and the v1 nibble codec (svb_half_encode_kernel, svb_half_decode_kernel), and the numpy
statement of both codecs: encode(), decode() ("32-bit un-zig-zag, 32-bit running sum, truncate on store": oracle/vbz_oracle.c,
generic_decompress) and build(), which lays a stream out from chosen 2-bit codes and chosen payloads -- how the rows are made that this
library's and the oracle's encoders never write: wide codes in a narrow type, padded codes, nibble code 3 with bits above 8, a last
byte whose unused nibble is not zero.  encoder_rows(kind) are values (the expected stream is the oracle's), decoder_rows(kind) are
streams (the expected bytes or verdict are the oracle's).  tests/test_generic_streams_ref.py holds the statement to the oracle and
counts what the catalogue contains; tests/test_gpu_generic_streams.py runs it on the device.  A plain module, no GPU, no oracle."""
import collections

import numpy as np

E_STREAM, E_DEST = 0xFFFFFFFB, 0xFFFFFFFC
M32 = 0xFFFFFFFF
# a kind: (bytes per value, zig-zag delta, vbz version); version 1 is the nibble codec for one-byte values only
KINDS = [(4, False, 0), (4, True, 0), (2, False, 0), (1, False, 0), (1, True, 0), (1, False, 1), (1, True, 1), (4, True, 1), (2, False, 1)]
DT = {1: np.int8, 2: np.int16, 4: np.int32}
# the 2-bit codes the kind's encoder can write
CODES = {(4, False): (0, 1, 2, 3), (4, True): (0, 1, 2, 3), (2, False): (0, 1, 3), (1, False): (0, 3), (1, True): (0, 1)}
EncRow = collections.namedtuple("EncRow", "name kind values marks")    # marks: what the row was built to hold (the ref test counts it)
DecRow = collections.namedtuple("DecRow", "name kind buf size cap tags")   # buf: the slot's bytes; size: src_size; cap: dst_cap (bytes)


def is_half(kind):
    return kind[0] == 1 and kind[2] == 1


def codes_of(kind):
    return (0, 1, 2, 3) if is_half(kind) else CODES[kind[:2]]


def geometry(size):
    """(V, W, T, G): values per lane (Vpl in svb_store.h), per wavefront, per tile, per segment (SEG_TILES = 8)"""
    V = 4 if size == 4 else 8
    return V, 64 * V, 256 * V, 8 * 256 * V


def kind_name(kind):
    return "int%d%s v%d" % (8 * kind[0], " zig-zag" if kind[1] else "", kind[2])


# ---- the statement ----------------------------------------------------------------------------------------------------------------------
def to_u(values, size, zigzag):
    """the 32-bit words the codec codes: the sign-extended values, or their zig-zag deltas (mod 2^32, the first against 0)"""
    x = np.asarray(values).astype(DT[size]).astype(np.int64)
    if not zigzag:
        return (x & M32).astype(np.uint64)
    d = (x - np.concatenate([[0], x[:-1]])) & M32
    return (((d << 1) & M32) ^ np.where(d >> 31, M32, 0)).astype(np.uint64)


def code_of(u, half):
    u = np.asarray(u, np.uint64)
    if half:
        return ((u != 0).astype(np.int64) + (u >= 16) + (u >= 256))
    return ((u > 0xFF).astype(np.int64) + (u > 0xFFFF) + (u > 0xFFFFFF))


def units(codes, half):
    """data units per value: bytes (code + 1), or nibbles ((1 << code) >> 1)"""
    codes = np.asarray(codes, np.int64)
    return (1 << codes) >> 1 if half else codes + 1


def stream_len(codes, half):
    n = int(units(codes, half).sum())
    return (len(codes) + 3) // 4 + ((n + 1) // 2 if half else n)


def build(codes, payloads, half):
    """the stream of len(codes) values: control bytes (four 2-bit codes each, the first in the low bits), then for every value the low
    bytes (nibbles, low nibble first) of its payload that its code announces"""
    codes, p = np.asarray(codes, np.int64), np.asarray(payloads, np.uint64)
    n = len(codes)
    K = (n + 3) // 4
    c4 = np.zeros(4 * K, np.int64)
    c4[:n] = codes
    keys = (c4[0::4] | c4[1::4] << 2 | c4[2::4] << 4 | c4[3::4] << 6).astype(np.uint8)
    m = units(codes, half)
    off = np.cumsum(m) - m
    total = int(m.sum())
    cells = np.zeros(total + 1, np.uint8)
    for j in range(4):
        sel = m > j
        cells[off[sel] + j] = ((p[sel] >> np.uint64((4 if half else 8) * j)) & np.uint64(0xF if half else 0xFF)).astype(np.uint8)
    if not half:
        return np.concatenate([keys, cells[:total]])
    cells = np.concatenate([cells[:total], np.zeros(total & 1, np.uint8)])
    return np.concatenate([keys, cells[0::2] | (cells[1::2] << 4)])


def encode(values, size, zigzag, half):
    u = to_u(values, size, zigzag)
    if len(u) == 0:
        return np.zeros(0, np.uint8)
    return build(code_of(u, half), u, half)


def decode(stream, count, size, zigzag, half):
    """the `count` values of `stream` (dtype DT[size]), or E_STREAM where the stream is not exactly what its control bytes announce"""
    stream = np.asarray(stream, np.uint8)
    if len(stream) == 0 or count == 0:
        return np.zeros(0, DT[size]) if len(stream) == count else E_STREAM
    K = (count + 3) // 4
    if K > len(stream):
        return E_STREAM
    codes = ((stream[:K, None] >> np.array([0, 2, 4, 6], np.uint8)) & 3).reshape(-1)[:count].astype(np.int64)
    m = units(codes, half)
    total = int(m.sum())
    if ((total + 1) // 2 if half else total) != len(stream) - K:
        return E_STREAM
    data = stream[K:].astype(np.uint64)
    cells = np.stack([data & np.uint64(0xF), data >> np.uint64(4)], 1).reshape(-1) if half else data
    cells = np.concatenate([cells, np.zeros(4, np.uint64)])
    off = np.cumsum(m) - m
    v = np.zeros(count, np.uint64)
    for j in range(4):
        v |= np.where(m > j, cells[off + j] << np.uint64((4 if half else 8) * j), np.uint64(0))
    if zigzag:
        d = (v >> np.uint64(1)) ^ np.where(v & np.uint64(1), np.uint64(M32), np.uint64(0))   # 32-bit un-zig-zag
        v = np.cumsum(d, dtype=np.uint64) & np.uint64(M32)                                   # 32-bit running sum
    return (v & np.uint64((1 << (8 * size)) - 1)).astype({1: np.uint8, 2: np.uint16, 4: np.uint32}[size]).view(DT[size])   # truncate on store


def verdict(stream, nbytes, kind):
    """decode() behind the capacity rule: the decoded bytes, or the error code"""
    size, zigzag, _ = kind
    if nbytes % size:
        return E_DEST
    got = decode(stream, nbytes // size, size, zigzag, is_half(kind))
    return got if isinstance(got, int) else got.view(np.uint8)


# ---- values with chosen codes -----------------------------------------------------------------------------------------------------------
U_RANGE = [(0, 0xFF), (0x100, 0xFFFF), (0x10000, 0xFFFFFF), (0x1000000, M32)]   # the words of each byte code


def _walk8_table():
    """[prev + 128][class]: the int8 values whose zig-zag delta from prev lies in the class, 0 left out (class 3 cannot leave 0)"""
    x = np.arange(-128, 128)
    table = []
    for prev in range(-128, 128):
        d = (x - prev) & M32
        cls = code_of(((d << 1) & M32) ^ np.where(d >> 31, M32, 0), True)
        table.append([x[(cls == c) & ((x != 0) | (c == 0))] for c in range(4)])
    return table


def walk8(classes, rng):
    """int8 values whose zig-zag deltas u lie in the given classes: 0: u = 0; 1: 1 ... 15; 2: 16 ... 255; 3: 256 ... 510, drawn from all
    values the class allows.  Class 3 from 0 (no int8 is 128 away) becomes class 2: the walk never returns to 0 once it has left it"""
    if "walk8" not in _cache:
        _cache["walk8"] = _walk8_table()
    table = _cache["walk8"]
    f = rng.random(len(classes))
    out = np.zeros(len(classes), np.int64)
    prev = 0
    for i, c in enumerate(classes.tolist()):
        cand = table[prev + 128][2 if c == 3 and prev == 0 else c]
        prev = int(cand[int(f[i] * len(cand))])
        out[i] = prev
    return out.astype(np.int8)


def values_for(kind, codes, rng):
    """values of the kind whose codes are `codes` (each one of codes_of(kind)), drawn over the whole range of each code"""
    size, zigzag, _ = kind
    half = is_half(kind)
    codes = np.asarray(codes, np.int64)
    n = len(codes)
    if size == 1 and zigzag:
        return walk8(codes if half else np.where(codes == 1, 3, rng.integers(0, 3, n)), rng)
    if size == 4:
        lo, hi = np.array(U_RANGE, np.int64).T
        u = rng.integers(lo[codes], hi[codes], endpoint=True)
        if zigzag:
            d = (u >> 1) ^ np.where(u & 1, M32, 0)
            u = np.cumsum(d) & M32
        return u.astype(np.uint32).view(np.int32)
    top = 127 if size == 1 else 32767
    if half:
        lo, hi = np.array([(0, 0), (1, 15), (16, 127), (-128, -1)], np.int64).T
    else:
        lo, hi = np.array([(0, min(255, top)), (256, top), (0, 0), (-top - 1, -1)], np.int64).T
    return rng.integers(lo[codes], hi[codes], endpoint=True).astype(DT[size])


def mix(kind, n, rng):
    """n values whose codes are drawn with equal odds from the codes the kind can write"""
    return values_for(kind, rng.choice(np.array(codes_of(kind)), n), rng)


# ---- encoder rows -----------------------------------------------------------------------------------------------------------------------
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def items(kind):
    """the boundary items of a kind: (name, prev, value) -- `value` stands at the marked position, `prev` (None: whatever is there) in
    front of it.  The word coded for `value` is the boundary the name says"""
    size, zigzag, _ = kind
    if not zigzag:
        if size == 4:
            vals = [0, 0xFF, 0x100, 0xFFFF, 0x10000, 0xFFFFFF, 0x1000000, -1, I32_MIN, I32_MAX]
        elif size == 2:
            vals = [0, 0xFF, 0x100, 0x7FFF, -1, -0x8000]
        else:
            vals = [0, 1, 15, 16, 127, -1, -128]
        out = [("%d" % v, None, v) for v in vals]
        if size != 4:
            out.append(("-1 behind the maximum", vals[-3] if size == 2 else 127, -1))
        return out
    if size == 4:
        out = [("delta %d" % d, 0, d) for d in (127, -128, 128, -32768, 32768, -(1 << 23), 1 << 23)]
        return out + [("INT32_MIN behind INT32_MAX", I32_MAX, I32_MIN), ("INT32_MAX behind INT32_MIN", I32_MIN, I32_MAX)]
    # (from 0 wherever an int8 can be that far from 0: those stand at a read's first value too)
    return [("u = 0", 0, 0), ("u = 1", 0, -1), ("u = 15", 0, -8), ("u = 16", 0, 8), ("u = 254", 0, 127), ("u = 255", 0, -128), ("u = 256", -64, 64),
            ("u = 510", -128, 127), ("u = 509", 127, -128)]


def spots(size, t):
    """(lane, slot) of the marked positions inside tile t: the tile's first value (which is the first of a wavefront's share, of the read
    for t = 0, of a segment for t % 8 = 0), lane 64's first (another wavefront's share), lanes 63 and 255, and every slot in a lane of its
    own.  No spot is the value in front of another, so a `prev` never lands on a mark"""
    V = geometry(size)[0]
    return [(0, 0), (64, 0), (63, V - 2), (255, V - 2)] + [(10 + 3 * k, k) for k in range(V)]


def quiet(kind, n, rng):
    size, zigzag, _ = kind
    if not zigzag:
        return rng.integers(1, 100, n).astype(DT[size])
    c = np.cumsum(rng.integers(-5, 6, n))
    return (np.abs((c + 40) % 160 - 80) - 40).astype(DT[size])   # (folded back at +-40: a step keeps its size)


def boundary_rows(kind, rng):
    """one row of 3 G + 5 values per item shift: tile t of row r holds item (t + r) % n at every spot, on a quiet background"""
    size = kind[0]
    V, W, T, G = geometry(size)
    its = items(kind)
    rows = []
    for r in range(len(its)):
        n = 3 * G + 5
        x = quiet(kind, n, rng).astype(np.int64)
        marks = []
        for t in range(n // T + 1):
            k = (t + r) % len(its)
            name, prev, value = its[k]
            for lane, slot in spots(size, t):
                p = t * T + lane * V + slot
                if p >= n or (p == 0 and prev not in (None, 0)):
                    continue
                x[p] = value
                if prev is not None and p > 0:
                    x[p - 1] = prev
                marks.append((k, p))
        rows.append(EncRow("boundaries, shift %d" % r, kind, x.astype(DT[size]), {"items": marks}))
    return rows


def mix_rows(kind, rng):
    size = kind[0]
    V, W, T, G = geometry(size)
    cs = codes_of(kind)
    rows = []
    if is_half(kind):
        rows.append(EncRow("code 0 only", kind, np.zeros(T + W + 3, np.int8), {"codes": [0]}))
        for parity in (1, 0):   # the total at every tile end is odd iff the first tile's is and every other tile's is even
            n = 3 * T + 5
            if kind[1]:   # 0, a1, 0, a3, ...: deltas +a, -a of as many nibbles (a != 8); a tile end's total has the parity of its last delta's
                a = rng.integers(1, 128, n)
                a[a == 8] = 9
                at = np.arange(T - 1, n, T)
                a[at] = rng.integers(1, 8, len(at)) if parity else rng.integers(9, 128, len(at))
                x = np.where(np.arange(n) % 2 == 1, a, 0)
            else:         # codes 1, 2 and 3 at random; a tile of the wrong parity gets its last value's code changed between 1 and 2
                codes = rng.integers(1, 4, n)
                for t in range(n // T):
                    if int(units(codes[t * T : (t + 1) * T], True).sum()) % 2 != (parity if t == 0 else 0):
                        codes[(t + 1) * T - 1] = 2 if codes[(t + 1) * T - 1] == 1 else 1
                x = values_for(kind, codes, rng)
            rows.append(EncRow("nibble total %s at every tile end" % ("odd" if parity else "even"), kind, x.astype(np.int8), {"parity": parity}))
        rows.append(EncRow("codes with equal odds", kind, mix(kind, 2 * T + 77, rng), {"mixed": True}))
        return rows
    # tiles that are all one length, each length the kind can write (a first value of int8 zig-zag cannot take two bytes: code 0 leads)
    order = list(cs) + list(cs)[::-1]
    codes = np.repeat(np.array(order), T)
    rows.append(EncRow("tiles of one length each", kind, values_for(kind, codes, rng), {"tiles": order}))
    rows.append(EncRow("lengths with equal odds", kind, mix(kind, 2 * T + 77, rng), {"mixed": True}))
    # the length switches exactly at a lane, a wavefront, a tile and a segment boundary
    cuts = [5 * V, 2 * W, 3 * T, G, G + T + W + 3 * V, 2 * G]
    n = 2 * G + T + 5
    codes = np.zeros(n, np.int64)
    for j, (a, b) in enumerate(zip([0] + cuts, cuts + [n])):
        codes[a:b] = cs[j % len(cs)]
    rows.append(EncRow("length switches at lane, wavefront, tile and segment boundaries", kind, values_for(kind, codes, rng), {"cuts": cuts}))
    return rows


def lengths(size):
    V, W, T, G = geometry(size)
    return [0, 1, V - 1, V, V + 1, W - 1, W, W + 1, T - 1, T, T + 1, 2 * T - 1, 2 * T + 1, G - 1, G, G + 1, 2 * G + 3, 3 * G + 5]


SEED = 97
_cache = {}


def _seed(kind, what):
    return [SEED, KINDS.index(kind), what]


def encoder_rows(kind):
    if ("enc", kind) not in _cache:
        rows = boundary_rows(kind, np.random.default_rng(_seed(kind, 0))) + mix_rows(kind, np.random.default_rng(_seed(kind, 1)))
        rng = np.random.default_rng(_seed(kind, 2))
        rows += [EncRow("%d values, codes with equal odds" % n, kind, mix(kind, n, rng), {"length": n}) for n in lengths(kind[0])]
        assert len({r.name for r in rows}) == len(rows)
        _cache["enc", kind] = rows
    return _cache["enc", kind]


# ---- decoder rows -----------------------------------------------------------------------------------------------------------------------
def stream_row(name, kind, stream, count, *tags):
    stream = np.ascontiguousarray(stream, np.uint8)
    return DecRow(name, kind, stream, len(stream), count * kind[0], frozenset(tags))


def foreign_rows(kind, rng):
    size, zigzag, _ = kind
    half = is_half(kind)
    V, W, T, G = geometry(size)
    full = np.uint64(0xFFFF if half else M32)
    rows = []

    def payload(n):   # over the whole width a code can announce: build() keeps the part the value's code does
        return rng.integers(0, int(full), n, endpoint=True).astype(np.uint64)

    for n in (T + 5, 2 * T, G + 1, 3 * G + 5):
        codes = ((rng.integers(0, 256, (n + 3) // 4)[:, None] >> np.array([0, 2, 4, 6])) & 3).reshape(-1)[:n]
        rows.append(stream_row("random control bytes, %d values" % n, kind, build(codes, payload(n), half), n, "foreign", "random"))
    for n in (T + 5, G + 1):   # values below 256 (the nibble codec: below 16) in more bytes (nibbles) than they need
        rows.append(stream_row("padded codes, %d values" % n, kind, build(rng.integers(1, 4, n), rng.integers(0, 16 if half else 256, n).astype(np.uint64), half),
                               n, "foreign", "padded"))
    if zigzag and not half:
        n = 2 * T   # deltas of about +2^30: the running sum passes 2^32 at every fourth value
        rows.append(stream_row("running sum passes 2^32", kind, build(np.full(n, 3), (rng.integers(1 << 29, 1 << 30, n) * 2).astype(np.uint64), half), n,
                               "foreign", "wraps"))
    if half:
        n = G + 1
        codes = np.where(rng.random(n) < 0.9, 3, rng.integers(0, 3, n))
        rows.append(stream_row("code 3 with bits 8 ... 15 set", kind, build(codes, payload(n) | np.uint64(0xA500), half), n, "foreign", "high bits"))
        for n in (T + 5, 3 * G + 5):
            codes = rng.integers(0, 4, n)
            if int(units(codes, True).sum()) % 2 == 0:
                codes[n - 1] = 1 if codes[n - 1] != 1 else 2
            s = build(codes, payload(n), half)
            assert int(units(codes, True).sum()) % 2 == 1 and s[-1] >> 4 == 0
            s[-1] |= 0xF0
            rows.append(stream_row("0xF in the unused nibble, %d values" % n, kind, s, n, "foreign", "unused nibble"))
    return rows


# defect -> (source size, capacity) of a stream of S bytes that holds n values of E bytes in K control bytes; "appended": one more byte in the slot
DEFECTS = {
    "intact": lambda S, n, K, E: (S, E * n),
    "last byte missing": lambda S, n, K, E: (S - 1, E * n),
    "one byte appended": lambda S, n, K, E: (S + 1, E * n),
    "src_size = K - 1": lambda S, n, K, E: (K - 1, E * n),
    "src_size = 0": lambda S, n, K, E: (0, E * n),
    "dst_cap + E": lambda S, n, K, E: (S, E * n + E),
    "dst_cap - E": lambda S, n, K, E: (S, E * n - E),
    "dst_cap + 1": lambda S, n, K, E: (S, E * n + 1),
    "dst_cap = 0": lambda S, n, K, E: (S, 0),
}


def defects_of(kind):
    return [d for d in DEFECTS if not (d == "dst_cap + 1" and kind[0] == 1)]   # (E = 1: that is dst_cap + E)


def defect_sizes(size):
    V, W, T, G = geometry(size)
    return [9, W + 1, T + 1, 2 * T + 5]


def defect_rows(kind, rng):
    size, zigzag, _ = kind
    half = is_half(kind)
    V, W, T, G = geometry(size)
    rows = []

    def add(n, names, parity=None, label=""):
        while True:   # (nibble codec: a read whose nibble total has the wanted parity)
            x = mix(kind, n, rng)
            u = to_u(x, size, zigzag)
            if parity is None or int(units(code_of(u, True), True).sum()) % 2 == parity:
                break
        stream = encode(x, size, zigzag, half)
        buf = np.concatenate([stream, np.zeros(1, np.uint8)])
        for name in names:
            s, cap = DEFECTS[name](len(stream), n, (n + 3) // 4, size)
            tags = {"defect", name, "n = %d" % n} | ({"nibbles odd" if parity else "nibbles even"} if parity is not None else set())
            rows.append(DecRow("%s, %d values%s" % (name, n, label), kind, buf, s, cap, frozenset(tags)))

    for j, n in enumerate(defect_sizes(size)):
        add(n, defects_of(kind), (1 - j % 2) if half else None)
    big = 2 * G + 1000   # three segments
    for j, name in enumerate(("last byte missing", "one byte appended", "dst_cap + E")):
        add(big, ("intact", name), j % 2 if half else None, " (read %d of three segments)" % j)
    return rows


def decoder_rows(kind):
    if ("dec", kind) not in _cache:
        size, zigzag, _ = kind
        rows = [stream_row(r.name, kind, encode(r.values, size, zigzag, is_half(kind)), len(r.values), "own") for r in encoder_rows(kind)]
        rows += foreign_rows(kind, np.random.default_rng(_seed(kind, 3))) + defect_rows(kind, np.random.default_rng(_seed(kind, 4)))
        assert len({r.name for r in rows}) == len(rows)
        _cache["dec", kind] = rows
    return _cache["dec", kind]
