"""The span entropy stage of the large-read path (vbz_compression_amd/csrc/zstd_encode.hip: span_cut, zstd_span_plan_kernel,
zstd_span_pack_kernel, zstd_span_finish_kernel) as a plain statement, the builder of reads whose svb stream has a chosen shape, and a
catalogue of such reads, one per seam and block kind.  Numpy and Python integers only; the constants are read from the sources, so
the statement follows them.  tests/test_span_frames_ref.py holds the builder to the oracle and counts what the catalogue contains,
tests/test_gpu_span_frames.py holds the device's frames to the statement.  A plain module: no GPU, no torch, no oracle.

The builder.  read_of(codes, data) is the int16 read whose zig-zag svb stream has exactly the given 2-bit code per sample (0: one data
byte, 1: two) and exactly the given data bytes, so K = ceil(T / 4) control bytes and D data bytes are set independently, to the byte,
and the data region holds any byte distribution.  read_of_i8 is the int8 zig-zag form (one byte per sample, D = T), read_of_u32 the
uint32 form without zig-zag (codes 0 ... 3).

The statement.  span_plan(N, K, shared_launch) lists the spans of a stream of N bytes with K control bytes, restated from
  span_cut                 zstd_encode.hip:1406-1416   which reads share tables, the two span limits, the empty frame
  zstd_span_plan_kernel    zstd_encode.hip:2832-2835   K of a read: (samples + 3) / 4, none below SPLIT_MIN stream bytes
                           zstd_encode.hip:2895-2909   span j of a region of n: [R j / n, R (j + 1) / n), the tree flag of the first shared span
  zstd_span_pack_kernel    zstd_encode.hip:2942, 2962-2966   blocks of a span: ceil(S / SPAN_BLOCK), base = S / nblk, the first S % nblk one longer
  zstd_span_finish_kernel  zstd_encode.hip:3031-3048   the index: only with more than one span, bit 31 = the last span is shared,
                                                       entry 0 = the frame header's length (5 + 1 / 2 / 4 for N < 256 / < 65792 / more)
and parse(frame) walks a compressed buffer: the frame without its trailers, the checkpoint trailer, the index and every block."""
import collections

import numpy as np

import sequences_ref as S

IDX_MAGIC, CP_MAGIC, ZSTD_MAGIC = 0x184D2A5C, 0x184D2A5B, 0xFD2FB528
SPLIT_MIN = S.SPLIT_MIN
SPAN_BLOCK = S._constant("zstd_encode.hip", r"#define VBZ_SPAN_BLOCK_KB (\d+)") << 10
SPAN_BYTES = SPAN_BLOCK * S._constant("zstd_encode.hip", r"#define VBZ_SPAN_SMALL_BLOCKS (\d+)")    # data spans with a table of their own
SHSPAN_BYTES = S._constant("zstd_encode.hip", r"constexpr uint32_t SHSPAN_BYTES = (\d+)u << (\d+)")   # data spans under a shared table
SHSPAN_BATCH_FROM = S._constant("zstd_encode.hip", r"SHSPAN_BATCH_FROM = (\d+)u << (\d+);")
SHSPAN_MIN_REGION = 2 * SHSPAN_BYTES      # zstd_encode.hip:122
SPAN_LARGE_FROM = S._constant("zstd_encode.hip", r"constexpr uint32_t SPAN_LARGE_FROM = (\d+)u << (\d+);")   # (out of this statement's range)
FHL_4 = 65536 + 256                       # stream bytes from which the frame header's content size takes four bytes
# vbz_api.hip:445-455, 465-471 (use_segments): a call takes the large-read path by its shape -- an encode from SMALL_BATCH_MIN_AVG raw bytes
# per read on (in a call of up to 96 MB), a decode of up to 64 frames from TINY_DECODE_MIN_AVG bytes of output per frame on
SMALL_BATCH_MIN_AVG = S._constant("vbz_api.hip", r"SMALL_BATCH_MIN_AVG = (\d+)u << (\d+)")
TINY_DECODE_MIN_AVG = S._constant("vbz_api.hip", r"TINY_DECODE_MIN_AVG = (\d+)u << (\d+)")
PLAN_ROUND = 1024                         # reads per round of zstd_span_plan_kernel (zstd_encode.hip:2821)

Span = collections.namedtuple("Span", "r0 r1 region shared tree")     # region: "key" or "data"; tree: the shared span that carries the table
Parsed = collections.namedtuple("Parsed", "body checkpoints flag entries header_len content_size blocks spans")
# blocks: [(frame offset, block type, literals type or None, Block_Size)]; spans: the blocks (type, literals type, size) under each index entry
Row = collections.namedtuple("Row", "name opts read codes data T K D N content raw_spans may_match tags")
# content: the data region's class; raw_spans: ordinals of the shared data spans that no table pays for; tags: what the row was built to hold

I16, I8, U32 = (True, 2, 1, 1), (True, 1, 1, 0), (False, 4, 1, 0)


# ---- the builder ------------------------------------------------------------------------------------------------------------------------
def _payloads(codes, data):
    codes, data = np.asarray(codes, np.int64), np.asarray(data, np.uint8)
    m = codes + 1
    assert int(m.sum()) == len(data), (int(m.sum()), len(data))
    off = np.cumsum(m) - m
    u = np.zeros(len(codes), np.uint64)
    padded = np.concatenate([data, np.zeros(4, np.uint8)]).astype(np.uint64)
    for j in range(4):
        u |= np.where(m > j, padded[off + j] << np.uint64(8 * j), np.uint64(0))
    top = padded[off + codes]
    assert bool((top[codes > 0] != 0).all()), "the high byte of a code of two bytes and more must not be zero"
    return u


def read_of(codes, data):
    """the int16 read whose zig-zag svb stream is these codes (0 / 1 per sample) and these data bytes"""
    assert len(codes) == 0 or int(np.max(codes)) <= 1
    u = _payloads(codes, data).astype(np.int64)
    d = (u >> 1) ^ -(u & 1)                                  # un-zig-zag
    return (np.cumsum(d) & 0xFFFF).astype(np.uint16).view(np.int16)


def read_of_i8(data):
    """the int8 read whose zig-zag svb stream is one data byte per sample, these; the walk must stay inside the type (the codec takes the
    difference of the sign-extended values, so a wrap would cost a second byte)"""
    u = np.asarray(data, np.uint8).astype(np.int64)
    x = np.cumsum((u >> 1) ^ -(u & 1))
    assert len(x) == 0 or (-128 <= int(x.min()) and int(x.max()) <= 127)
    return x.astype(np.int8)


def read_of_u32(codes, data):
    """the uint32 read (no zig-zag) whose svb stream is these codes (0 ... 3) and these data bytes"""
    return _payloads(codes, data).astype(np.uint32)


def control_bytes(codes):
    c4 = np.zeros((len(codes) + 3) // 4 * 4, np.int64)
    c4[: len(codes)] = codes
    return (c4[0::4] | c4[1::4] << 2 | c4[2::4] << 4 | c4[3::4] << 6).astype(np.uint8)


def stream_of(codes, data):
    return np.concatenate([control_bytes(codes), np.asarray(data, np.uint8)])


# ---- the statement ----------------------------------------------------------------------------------------------------------------------
def key_bytes(N, T):
    """the control bytes the plan cuts off a stream of N bytes and T samples (zstd_encode.hip:2832-2835)"""
    K = (T + 3) // 4 if N >= SPLIT_MIN else 0
    return 0 if K >= N else K


def span_plan(N, K, shared_launch):
    """[Span] of a stream of N bytes, the first K of them control bytes, in a launch with (without) the shared-table kernels"""
    assert N < SPAN_LARGE_FROM and K <= N
    if N == 0:
        return [Span(0, 0, "data", False, False)]            # the empty frame is one span (zstd_encode.hip:1415)
    D = N - K
    shared = bool(shared_launch and K and D >= SHSPAN_MIN_REGION)
    limit = SHSPAN_BYTES if shared else SPAN_BYTES
    n = (D + limit - 1) // limit
    out = [Span(a, b, "key", False, False) for a, b in S.key_spans(K, shared=bool(shared_launch))]
    return out + [Span(K + D * t // n, K + D * (t + 1) // n, "data", shared, shared and t == 0) for t in range(n)]


def span_count(N, K, shared_launch):
    """the closed form of len(span_plan(...))"""
    if N == 0:
        return 1
    D = N - K
    shared = bool(shared_launch and K and D >= SHSPAN_MIN_REGION)
    kl = S.KEYSPAN_SHARED if shared_launch else (2 * S.KEYSPAN if K >= S.KEYSPAN_LARGE_FROM else S.KEYSPAN)
    dl = SHSPAN_BYTES if shared else SPAN_BYTES
    return -(-K // kl) + -(-D // dl)


def block_sizes(size):
    """the content of the blocks of a span of `size` bytes that is packed with a table or stored raw by zstd_span_pack_kernel"""
    n = (size + SPAN_BLOCK - 1) // SPAN_BLOCK
    return [size // n + (1 if j < size % n else 0) for j in range(n)]


def header_len(N):
    return 5 + (1 if N < 256 else 2 if N < FHL_4 else 4)


def index_of(plan, N):
    """(flag, content offsets) of the index the finish kernel writes, or None for a frame of one span"""
    if len(plan) < 2:
        return None
    return bool(plan[-1].shared), [s.r0 for s in plan]


def trailer(magic, words):
    """the skippable frame of these payload words: magic, payload bytes, the words, the trailer's own size"""
    tb = 8 + 4 * len(words) + 4
    return np.array([magic, tb - 8] + list(words) + [tb], "<u4").view(np.uint8)


def parse(frame):
    """Parsed of one compressed buffer (unsized): the skippable frames are found from the end, each by its last word (its size), its magic
    and its payload length; the blocks by their 3-byte headers (last | type << 1 | size << 3; an RLE block holds one byte)"""
    f = np.asarray(frame, np.uint8)
    found = {}
    while len(f) >= 24:
        tb = int(f[-4:].view("<u4")[0])
        if tb < 16 or tb > len(f) - 9:
            break
        m = f[len(f) - tb : len(f) - tb + 8].view("<u4")
        if int(m[0]) not in (IDX_MAGIC, CP_MAGIC) or int(m[1]) != tb - 8 or int(m[0]) in found:
            break
        found[int(m[0])] = f[len(f) - tb :]
        f = f[: len(f) - tb]
    assert int(f[:4].view("<u4")[0]) == ZSTD_MAGIC
    fhd = int(f[4])
    assert fhd & 0x20 and not fhd & 0x0F, hex(fhd)          # single segment, no checksum, no dictionary: the library's frames
    fcs = (1, 2, 4, 8)[fhd >> 6]
    content = int.from_bytes(f[5 : 5 + fcs].tobytes(), "little") + (256 if fcs == 2 else 0)
    blocks, pos = [], 5 + fcs
    while True:
        h = int(f[pos]) | int(f[pos + 1]) << 8 | int(f[pos + 2]) << 16
        bt, size = (h >> 1) & 3, h >> 3
        blocks.append((pos, bt, int(f[pos + 3]) & 3 if bt == 2 else None, size))
        pos += 3 + (1 if bt == 1 else size)
        if h & 1:
            break
    assert pos == len(f), (pos, len(f))
    flag, entries, spans = None, None, None
    if IDX_MAGIC in found:
        w = found[IDX_MAGIC].view("<u4")
        ns = int(w[2]) & 0x7FFFFFFF
        assert len(w) == 4 + 2 * ns, (len(w), ns)
        flag, entries = bool(int(w[2]) >> 31), [(int(w[3 + 2 * j]), int(w[4 + 2 * j])) for j in range(ns)]
        ends = [e[0] for e in entries[1:]] + [len(f)]
        spans = [[b[1:] for b in blocks if entries[j][0] <= b[0] < ends[j]] for j in range(ns)]
    return Parsed(f, found.get(CP_MAGIC), flag, entries, 5 + fcs, content, blocks, spans)


# ---- the catalogue ----------------------------------------------------------------------------------------------------------------------
def skewed(rng, n, nonzero=False):
    """n i.i.d. draws of a skewed alphabet (~5.5 bits per byte: a table pays, and no 16-byte window occurs twice in 100 KB); nonzero: of
    the byte values 1 ... 255, for the regions of reads with two-byte codes"""
    p = 0.97 ** np.arange(256)
    sym = rng.permutation(256 - nonzero) + nonzero
    return sym[rng.choice(len(sym), n, p=p[: len(sym)] / p[: len(sym)].sum())].astype(np.uint8)


def row_of(name, opts, codes, data, content="skewed", raw_spans=(), may_match=False, tags=()):
    codes, data = np.asarray(codes, np.int64), np.asarray(data, np.uint8)
    read = read_of_u32(codes, data) if opts == U32 else read_of_i8(data) if opts == I8 else read_of(codes, data)
    T, D = len(codes), len(data)
    N = (T + 3) // 4 + D
    return Row(name, opts, read, codes, data, T, key_bytes(N, T), N - key_bytes(N, T), N, content, tuple(raw_spans), may_match, tuple(tags))


def _geometry(rng, T, D, tag, opts=I16):
    """T samples and D data bytes of the skewed alphabet: the first D - T samples take two bytes (int16; uint32: codes 0 ... 3 that add up)"""
    if opts == I8:
        assert D == T
        v = rng.integers(-64, 64, T)                        # values whose differences fit a byte
        d = np.diff(np.concatenate([[0], v]))
        return row_of("%s T=%d D=%d int8" % (tag, T, D), opts, np.zeros(T, np.int64), ((d << 1) ^ (d >> 63)).astype(np.uint8), tags=(tag,))
    codes = np.zeros(T, np.int64)
    if opts == U32:
        extra = D - T
        codes[: extra // 3] = 3
        codes[extra // 3] = extra % 3
    else:
        codes[: D - T] = 1
    return row_of("%s T=%d D=%d%s" % (tag, T, D, " uint32" if opts == U32 else ""), opts, codes, skewed(rng, D, nonzero=True), tags=(tag,))


def geometry_rows():
    rng = np.random.default_rng(4601)
    rows = [row_of("empty", I16, [], [], content="none", tags=("empty",)), row_of("one sample", I16, [0], [7], content="none", tags=("one",))]
    rows += [_geometry(rng, 1600, N - 400, "N=2048") for N in (2047, 2048, 2049)]                 # the control-byte region appears
    rows += [_geometry(rng, 52000, N - 13000, "N=65792") for N in (65791, 65792)]                 # the frame header grows under an index
    rows += [_geometry(rng, 16000, D, "D=16384") for D in (16383, 16384, 16385)]                  # unshared 1 span, shared 2, shared 3
    rows += [_geometry(rng, 16000, 8192 * 3 + e, "D=8192m") for e in (-1, 0, 1)]
    rows += [_geometry(rng, 20000, 8192 * 4 + e, "D=8192m") for e in (-1, 0, 1)]                  # (and 32 768 / 32 769 unshared: one span or two)
    rows += [_geometry(rng, T, 20000, "K=4096") for T in (16384, 16385)]
    rows += [_geometry(rng, T, 40000, "K=8192") for T in (32768, 32769)]
    rows += [_geometry(rng, 10000, D, "u32 D=16384", U32) for D in (16384, 16385)]                # unshared by type: one block or two
    rows += [_geometry(rng, 10000, D, "u32 D=32768", U32) for D in (32768, 32769)]                # ... one span or two
    rows += [_geometry(rng, D, D, "i8 D=16384", I8) for D in (16383, 16384)]
    return rows


def _rare_first(rng, D, nspans):
    """D bytes of 256 symbols: 200 rare ones, each ~1 / 1200 of the region, make up the whole first span; 56 common ones the rest"""
    sym = rng.permutation(256)
    head = D // nspans
    rest = sym[200 + rng.choice(56, D - head, p=(0.93 ** np.arange(56)) / (0.93 ** np.arange(56)).sum())]
    return np.concatenate([sym[rng.integers(0, 200, head)], rest]).astype(np.uint8)


def content_rows():
    """data-region classes, codes all 0 (D = T: no constraint on any byte), D = 5 shared spans unless said otherwise"""
    rng = np.random.default_rng(4602)
    D, n = 40000, 5
    cut = [D * t // n for t in range(n + 1)]

    def row(name, data, **kw):
        return row_of(name, I16, np.zeros(len(data), np.int64), data, tags=(kw.get("content", "skewed"),), **kw)

    rows = [row("uniform bytes", rng.integers(0, 256, D), content="uniform", raw_spans=range(n))]
    rows.append(row("rarest symbols first", _rare_first(rng, 6 * 8000, 6), content="rare first"))
    for at, where in ((1, "behind the tree span"), (2, "in the middle"), (n - 1, "last")):
        d = skewed(rng, D)
        d[cut[at] : cut[at + 1]] = rng.integers(0, 256, cut[at + 1] - cut[at])
        rows.append(row("one uniform span " + where, d, content="uniform span", raw_spans=(at,)))
    d = skewed(np.random.default_rng(7), D)
    absent = int(np.flatnonzero(np.bincount(d, minlength=256) == np.bincount(d, minlength=256).min())[0])
    d[d == absent] = d[0] if d[0] != absent else d[1]
    d[D - 100] = absent
    rows.append(row("a symbol once, in the last span", d, content="once"))
    d = skewed(rng, D)
    d[cut[2] : cut[3]] = d[0]
    rows.append(row("one span of one symbol", d, content="constant span", may_match=True))
    rows.append(row("two symbols", np.array([3, 200], np.uint8)[rng.integers(0, 2, D)], content="two symbols", may_match=True))
    rows.append(row("one byte value", np.full(D, 0x41, np.uint8), content="one value", may_match=True))
    return rows


def huffman_lengths(hist):
    """the code lengths of an optimal prefix code for these counts (0 for a symbol that does not occur)"""
    import heapq

    heap = [(int(c), i, (i,)) for i, c in enumerate(hist) if c]
    heapq.heapify(heap)
    length = np.zeros(len(hist), np.int64)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        length[list(a[2] + b[2])] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    return length


GRADIENT_SPAN, GRADIENT_SPANS, GRADIENT_FLAT, GRADIENT_STEP = 8000, 40, 16, 96


def gradient_row():
    """40 shared spans of 8000 bytes: the first 16 of a skewed alphabet (they keep the region's table skewed), span t behind them of u(t)
    uniform bytes among 8000 - u(t) skewed ones, u rising by 96 a span, so that what a span costs under the region's table rises by
    ~20 bytes a span, through its own size: the spans in front of the crossing stay treeless, the ones behind it are stored raw, and
    one of them comes within a few dozen bytes of the fallback's bound (zstd_encode.hip:2950) whichever side it falls"""
    rng = np.random.default_rng(4606)
    S, n, flat = GRADIENT_SPAN, GRADIENT_SPANS, GRADIENT_FLAT
    mid = (flat + n) // 2
    p = 0.97 ** np.arange(256)
    sym = rng.permutation(256)

    def make(c):
        spans = [sym[rng.choice(256, S, p=p / p.sum())] for _ in range(flat)]
        for t in range(flat, n):
            u = c + GRADIENT_STEP * (t - mid)
            spans.append(rng.permutation(np.concatenate([rng.integers(0, 256, u), sym[rng.choice(256, S - u, p=p / p.sum())]])))
        return np.concatenate(spans).astype(np.uint8)

    c = S // 2
    for _ in range(4):       # place the middle span's cost at its size (+ 20: the block's headers)
        cost = gradient_costs(make(c))
        per_step = (cost[-1] - cost[flat]) / (n - 1 - flat)
        c += round((S + 20 - cost[mid]) / per_step) * GRADIENT_STEP
        c = int(min(max(c, GRADIENT_STEP * (mid - flat)), S - GRADIENT_STEP * (n - mid)))
    d = make(c)
    return row_of("gradient through the fallback's bound", I16, np.zeros(len(d), np.int64), d, content="gradient", tags=("gradient",))


def gradient_costs(data):
    """bytes of Huffman streams each span of the gradient row's region takes under an optimal code for the region"""
    length = huffman_lengths(np.bincount(data, minlength=256))
    return [int(length[data[GRADIENT_SPAN * t : GRADIENT_SPAN * (t + 1)]].sum()) / 8 for t in range(GRADIENT_SPANS)]


KEY_K = 8193


def _key_row(rng, name, zero_from, zero_to):
    """K = 8193 control bytes: random codes except in the control bytes [zero_from, zero_to), which are zero"""
    T = 4 * KEY_K
    codes = rng.integers(0, 2, T)
    codes[4 * zero_from : 4 * zero_to] = 0
    codes[4 * zero_from - 1] = codes[4 * zero_to] = 1       # (the run is exactly this long)
    return row_of(name, I16, codes, skewed(rng, int(T + codes.sum()), nonzero=True))


def key_rows():
    rng = np.random.default_rng(4603)
    T = 4 * KEY_K
    rows = [row_of("keys all zero", I16, np.zeros(T, np.int64), skewed(rng, T), tags=("keys", "keys zero"))]
    for shared in (True, False):   # the first seam of the key spans of either launch kind
        seam = S.key_spans(KEY_K, shared=shared)[0][1]
        rows.append(_key_row(rng, "zero run ends on seam %d" % seam, seam - 600, seam)._replace(tags=("keys", "run ends on", seam)))
        rows.append(_key_row(rng, "zero run crosses seam %d" % seam, seam - 300, seam + 300)._replace(tags=("keys", "run crosses", seam)))
    codes = np.zeros(T, np.int64)
    codes[83::84] = 1                       # every 21st control byte is not zero: ~195 zero runs, each a sequence, in every 4 KB of them
    rows.append(row_of("keys in zero runs", I16, codes, skewed(rng, int(T + codes.sum()), nonzero=True), tags=("keys", "keys runs")))
    rows.append(row_of("keys without a zero", I16, np.ones(T, np.int64), skewed(rng, 2 * T, nonzero=True), tags=("keys", "keys no zero")))
    return rows


def large_key_rows():
    """K = 2^20 - 1 / 2^20 (KEYSPAN_LARGE_FROM: the key spans double in a launch without shared tables); 8 MB of samples each"""
    rng = np.random.default_rng(4604)
    return [row_of("K=%d" % ((T + 3) // 4), I16, np.zeros(T, np.int64), skewed(rng, T), tags=("K=2^20",)) for T in (4 * S.KEYSPAN_LARGE_FROM - 4, 4 * S.KEYSPAN_LARGE_FROM)]


_rows = []


def rows():
    """the catalogue (built once): geometry rows, data-region content rows, control-byte content rows"""
    if not _rows:
        _rows.extend(geometry_rows() + content_rows() + [gradient_row()] + key_rows())
        assert len({r.name for r in _rows}) == len(_rows)
    return _rows


def launch_shared(opts, shared_tables=True):
    """whether a call of less than SHSPAN_BATCH_FROM bytes of stream bound is a shared launch (vbz_api.hip:638: one- and two-byte integers)"""
    return bool(shared_tables and opts[1] in (1, 2))


def expected_kinds(row, plan):
    """what the statement says of every span of a row's frame: "key", or for a data span one of
    "tree" (its first block is compressed and carries a tree), "treeless" (every block compressed, treeless), "raw", "rle", "either"
    (treeless or raw, whichever is shorter: the gradient row), "own" (a span with a table of its own: its first block carries its tree), "own or raw" (... or one raw block)"""
    out, t = [], 0
    for s in plan:
        if s.region == "key":
            out.append("key")
            continue
        if not s.shared:
            mixed = row.content in ("uniform span", "gradient")      # some of its 32 KB may not pay for a table: the span's own decision
            out.append("raw" if row.content == "uniform" else "rle" if row.content == "one value" else "own or raw" if mixed else "own")
        elif row.content == "uniform":
            out.append("raw")
        elif row.content == "one value":
            out.append("rle")
        else:
            out.append("tree" if s.tree else "either" if row.content == "gradient" else "raw" if t in row.raw_spans else "treeless")
        t += 1
    return out
