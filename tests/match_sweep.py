"""The sweep of the signal-match kernels (csrc/match.hip) beside the catalogues of match_ref, match_span_ref and match_path_ref: which
loop of match.hip a pair runs, restated from the two host headers, the census of what a set of calls reaches, and the calls that reach
the rest -- a dense sweep of small (n, M, W) with garbage behind every end, one reference per (rows per lane, tracked row), paths for
every class on both keys, stretched copies that make the traceback refetch inside one lane's stream, and the packed key's bound with both
of its fields full.  Built from match_ref.Call and match_path_ref.PathCall; the existing catalogues are not touched (they are seeded: a
draw added in their middle moves every expected value).  A plain module: tests/test_match_sweep_host.py holds it on the CPU,
tests/test_gpu_match_sweep.py runs it on the device."""
import functools

import numpy as np

import match_path_ref as P
import match_ref as M
import match_span_ref as S

CS = (1, 2, 4, 8, 16, 32)
COST, SPAN, SPAN_WIDE, PATH, PATH_WIDE = ("match_kernel", "match_span_kernel", "match_span_wide_kernel", "match_path_forward_kernel",
                                          "match_path_forward_wide_kernel")


# ---- 1. the dispatch of match.hip, restated -----------------------------------------------------------------------------------------------
def rows_per_lane(rows):
    """csrc/match_path_groups.h: match_rows_per_lane -- the smallest of 1, 2, 4, 8, 16, 32 with 64 c >= rows"""
    c = 1
    while c < 32 and 64 * c < rows:
        c *= 2
    return c


def start_bits(N):
    """csrc/match_select.h: match_span_start_bits -- ceil(log2 N)"""
    sb = 0
    while (1 << sb) < N:
        sb += 1
    return sb


def packed(N, stride):
    """csrc/match_select.h: match_span_packed"""
    sb = start_bits(N)
    return sb <= 16 and 255 * stride < (1 << (31 - sb))


def match_path_pair_bytes(max_width, stride):
    """csrc/match_path_groups.h: match_path_pair_words, in bytes -- the direction bits one pair of a path call takes"""
    return 4 * 64 * (((63 + max_width) * rows_per_lane(stride) + 15) // 16)


def instantiation(kind, N, stride, m):
    """(kernel, C, SEL) of a pair whose reference has m levels.  kind "cost", "span" (N: query_len) or "path" (N: max_width).  SEL: the
    tracked row of the span kernels -- (m - 1) mod C packed, the lane's last row wide -- and None where no loop is chosen by it"""
    c = rows_per_lane(m)
    if kind == "cost":
        return COST, c, None
    if kind == "span":
        return (SPAN, c, (m - 1) % c) if packed(N, stride) else (SPAN_WIDE, c, c - 1)
    assert kind == "path"
    return (PATH if packed(N, stride) else PATH_WIDE), c, None


# ---- 2. what a call runs ------------------------------------------------------------------------------------------------------------------
class Shape:
    """what the census needs of one launch: kind, N (max_width of a path call), ref_stride and the (n, M) -- (W, M) of a path call -- of
    every pair that reaches a loop (n, W >= 1, 1 <= M <= stride)"""

    def __init__(self, name, kind, N, stride, pairs):
        self.name, self.kind, self.N, self.stride, self.pairs = name, kind, N, stride, [(int(n), int(m)) for n, m in pairs if n > 0]

    def at(self, name, N=None, stride=None):
        """the same pairs at another (N, stride): the wide twin of a call"""
        return Shape(name, self.kind, self.N if N is None else N, self.stride if stride is None else stride, self.pairs)


def call_shapes(call, kinds=("cost", "span")):
    return [Shape(call.name, kind, call.N, call.stride, call.pairs()) for kind in kinds]


def path_pairs(pc):
    """(pair index, W, M) of the pairs of a PathCall that pass the header's conditions"""
    c = pc.call
    out = []
    for p, (rd, rf, a, b) in enumerate(pc.pairs):
        if rd >= len(c.rows) or rf >= len(c.refs) or a >= b:
            continue
        n, m = min(int(c.valid[rd]), c.N), int(c.ref_len[rf])
        if b > n or b - a > pc.max_width or m == 0 or m > c.stride:
            continue
        out.append((p, b - a, m))
    return out


def path_shape(pc):
    return Shape(pc.name, "path", pc.max_width, pc.call.stride, [(w, m) for _, w, m in path_pairs(pc)])


def census(shapes):
    """{(kernel, C, SEL): set of steps = n + la the loop ran over}"""
    out = {}
    for s in shapes:
        for n, m in s.pairs:
            inst = instantiation(s.kind, s.N, s.stride, m)
            out.setdefault(inst, set()).add(n + (m - 1) // inst[1])
    return out


def long_runs(pc, rows):
    """{(kernel, C): the most columns one reference row holds in the rule's path} over the pairs of a PathCall, from match_path_ref's rows
    (uint32 [pairs, stride, 2]).  The traceback serves 1 024 cells -- 1 024 / C columns -- from one fetch of a lane's stream, so a row
    that holds more than (1 024 + 16) / C columns makes it refetch inside that stream whatever the word's phase is"""
    out = {}
    for p, w, m in path_pairs(pc):
        kernel, c, _ = instantiation("path", pc.max_width, pc.call.stride, m)
        r = rows[p, :m].astype(np.int64)
        out[(kernel, c)] = max(out.get((kernel, c), 0), int((r[:, 1] - r[:, 0]).max()))
    return out


# (N, ref_stride, M) of the span launches of the fused-call tests (test_gpu_match_span.py: refs_from and the python methods), which run
# no catalogue: stretches of the queries themselves, plateaus of 400, a small alphabet of 33, a constant of 20
FUSED = [(512, 416, 150), (512, 416, 211), (512, 416, 400), (512, 416, 33), (256, 416, 150), (256, 416, 211), (256, 416, 400), (256, 416, 33),
         (256, 64, 40), (256, 64, 64), (256, 64, 9)]


def existing_shapes():
    """the launches of the suite before the sweep: both cost and span over match_ref's catalogue, span (and its cost-only cross-check) over
    match_span_ref's, path over match_path_ref's, and the fused calls' references against a read that fills its row"""
    out = []
    for c in M.catalogue():
        out += call_shapes(c)
    for c in S.span_catalogue():
        out += call_shapes(c)
    for N, stride, m in FUSED:
        out += [Shape("fused", kind, N, stride, [(N, m)]) for kind in ("cost", "span")]
    out += [path_shape(pc) for pc in P.catalogue()]
    return out


def existing_lengths():
    """every reference length the suite held before the sweep"""
    held = {m for s in existing_shapes() for _, m in s.pairs}
    return held | set(M.LENGTHS_M) | set(S.TIE_M) | set(S.TIE_SHORT)


# ---- 3. the calls -------------------------------------------------------------------------------------------------------------------------
GARBAGE = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 127.0, -127.0, 3.0, -64.0, 0.5, -1.5, 200.0], np.float32)


def _tail(rng, length):
    """query entries behind a read's end: NaN, infinities, +-1e30 and levels inside the range -- whatever a kernel that read one entry
    too far would NOT get away with (the catalogues pad with +0)"""
    return GARBAGE[rng.integers(0, len(GARBAGE), length)]


def _fill(call, seed):
    """garbage behind every read's valid count and every reference's length, in place (refused lengths: the whole row)"""
    rng = np.random.default_rng(seed)
    for row, v in zip(call.rows, call.valid):
        n = min(int(v), call.N)
        row[n:] = _tail(rng, call.N - n)
    for row, m in zip(call.refs, call.ref_len):
        m = int(m) if 0 < int(m) <= call.stride else 0
        row[m:] = rng.integers(-128, 128, call.stride - m)
        if m + 1 < call.stride:
            row[m + int(rng.integers(0, 2))] = -128
    return call


def widen(call, N=None, stride=None, seed=77):
    """the same reads and references in an arena of another (N, stride) -- the twin that runs the other kernel.  What is behind the ends,
    old and new, is garbage again"""
    w = M.Call(call.name + "-wide", call.N if N is None else N, call.quant, call.stride if stride is None else stride)
    assert w.N >= call.N and w.stride >= call.stride
    for row, v in zip(call.rows, call.valid):
        x = np.zeros(w.N, np.float32)
        x[: call.N] = row
        w.rows.append(x)
        w.valid.append(v)
    for row, m in zip(call.refs, call.ref_len):
        x = np.zeros(w.stride, np.int8)
        x[: call.stride] = row
        w.refs.append(x)
        w.ref_len.append(m)
    return _fill(w, seed)


def _levels(rng, n):
    """odd n: three levels, where paths tie; even n: signal"""
    return rng.integers(-1, 2, n) if n % 2 else M._signal_levels(rng, n)


# A. dense: every n = 1 ... 136 against every M = 1 ... 136
DENSE_N, DENSE_STRIDE, DENSE_MAX = 136, 144, 136
DENSE_WIDE_N = 65536


@functools.lru_cache(maxsize=None)
def dense(garbage=True):
    rng = np.random.default_rng(5310)
    a = M.Call("dense", DENSE_N, 1.0, DENSE_STRIDE)
    for n in range(1, DENSE_MAX + 1):
        a.read(_levels(rng, n))
    for m in range(1, DENSE_MAX + 1):
        a.ref(_levels(rng, m))
    return _fill(a, 5311) if garbage else a


def _frozen(*arrays):
    for x in arrays:
        x.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _hits(call):
    query, valid, ref, ref_len = call.arrays()
    return _frozen(M.hits(query, valid, call.quant, ref, ref_len))


def _spans(call):
    query, valid, ref, ref_len = call.arrays()
    return _frozen(S.spans(query, valid, call.quant, ref, ref_len))


@functools.lru_cache(maxsize=None)
def dense_hits():
    return _hits(dense())


@functools.lru_cache(maxsize=None)
def dense_spans(garbage=True):
    return _spans(dense(garbage))


# B. every instantiation of the packed span kernel: one M per (C, SEL)
EVERY_N, EVERY_WIDE_N, EVERY_STRIDE = 256, 8192, 2048
EVERY_READS = (256, 255, 130, 129, 64, 1)


@functools.lru_cache(maxsize=None)
def every_lengths():
    """one M per (C, SEL) from the upper half of its class -- la = 48 ... 63 (C = 1: 32 ... 63) -- away from every M the suite held.  For
    C >= 8 the reference of SEL 0 takes la = 63: against n = 129 and 130 its steps are 192 and 193, both parities and both sides of a
    block of 64"""
    rng = np.random.default_rng(5320)
    held, out = existing_lengths(), []
    for c in CS:
        for sel in range(c):
            for _ in range(1000):
                la = 63 if c >= 8 and sel == 0 else int(rng.integers(32 if c == 1 else 48, 64))
                m = la * c + sel + 1
                if m not in held and m not in out:
                    break
            else:
                raise AssertionError((c, sel))
            out.append(m)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def every():
    rng = np.random.default_rng(5321)
    b = M.Call("every", EVERY_N, 32.0, EVERY_STRIDE)
    for n in EVERY_READS:
        b.read(M._signal_levels(rng, n))
    for m in every_lengths():
        b.ref(M._signal_levels(rng, m))
    return _fill(b, 5322)


@functools.lru_cache(maxsize=None)
def every_spans():
    return _spans(every())


@functools.lru_cache(maxsize=None)
def every_hits():
    return _hits(every())


# C. dense paths: every M = 1 ... 136 against every W = 1 ... 34 over the two longest reads of A
PATHS_MAX_W, PATHS_WIDTH, PATHS_WIDE = 34, 40, 32776   # (32 776 x 144 is the smallest wide shape: 255 x 144 >= 2^15)


def _path_call(name, base, reads, N, max_width, stride=None, seed=78):
    """a PathCall over rows `reads` of `base` (renumbered from 0) and all its references, in an arena of (N, stride)"""
    pc = P.PathCall(name, N, base.quant, base.stride if stride is None else stride, max_width)
    sub = M.Call(name, base.N, base.quant, base.stride)
    sub.rows, sub.valid = [base.rows[i] for i in reads], [base.valid[i] for i in reads]
    sub.refs, sub.ref_len = base.refs, base.ref_len
    pc.call = sub if (N, pc.call.stride) == (base.N, base.stride) else widen(sub, N, pc.call.stride, seed)
    pc.call.name = name
    return pc


@functools.lru_cache(maxsize=None)
def dense_paths():
    """read 0: n = 136, signal; read 1: n = 135, three levels.  a is drawn, so it is mostly a multiple of nothing"""
    rng = np.random.default_rng(5330)
    pc = _path_call("dense-paths", dense(), (DENSE_MAX - 1, DENSE_MAX - 2), DENSE_N, PATHS_WIDTH)
    for m in range(1, DENSE_MAX + 1):
        for w in range(1, PATHS_MAX_W + 1):
            rd = int(rng.integers(0, 2))
            n = DENSE_MAX - rd
            a = int(rng.integers(0, n - w + 1))
            pc.pair(rd, m - 1, a, a + w)
    return pc


@functools.lru_cache(maxsize=None)
def dense_paths_expected():
    pc = dense_paths()
    query, valid, ref, ref_len = pc.call.arrays()
    return _frozen(*P.paths(query, valid, pc.call.quant, ref, ref_len, pc.pairs, pc.max_width))


PATHS_WIDE_SEAMS = (1, 64, 65, 128, 129, 136)   # every W = 1 ... 16, 33 and 34 for these M: every phase of the open word for C = 1, 2, 4


@functools.lru_cache(maxsize=None)
def dense_paths_wide_pick():
    """the pairs of dense_paths() the wide twin runs, at most 256: one per M, and for the M of PATHS_WIDE_SEAMS 18 widths"""
    rng = np.random.default_rng(5331)
    pick = [(m - 1) * PATHS_MAX_W + int(rng.integers(0, PATHS_MAX_W)) for m in range(1, DENSE_MAX + 1)]
    for m in PATHS_WIDE_SEAMS:
        pick += [(m - 1) * PATHS_MAX_W + w - 1 for w in list(range(1, 17)) + [33, 34]]
    pick = tuple(sorted(set(pick)))
    assert len(pick) <= 256
    return pick


def dense_paths_wide():
    pc = _path_call("dense-paths-wide", dense(), (DENSE_MAX - 1, DENSE_MAX - 2), PATHS_WIDE, PATHS_WIDE)
    pc.pairs = [dense_paths().pairs[p] for p in dense_paths_wide_pick()]
    return pc


# D. paths per class: two references for every C >= 2 against widths around the blocks of 64 steps
CLASS_N, CLASS_WIDE_N, CLASS_STRIDE = 256, 8192, 2048
CLASS_WIDTHS = (1, 2, 63, 64, 65, 129, 200, 256)


@functools.lru_cache(maxsize=None)
def class_paths(wide=False):
    rng = np.random.default_rng(5340)
    base = M.Call("class-paths", CLASS_N, 32.0, CLASS_STRIDE)
    base.read(M._signal_levels(rng, CLASS_N))
    held = existing_lengths() | set(every_lengths())
    for c in CS[1:]:
        base.ref(M._signal_levels(rng, 64 * c))   # the top of the class: la = 63
        m = int(rng.integers(32 * c + 1, 64 * c))
        while m in held:
            m = int(rng.integers(32 * c + 1, 64 * c))
        base.ref(M._signal_levels(rng, m))
    _fill(base, 5341)
    N = CLASS_WIDE_N if wide else CLASS_N
    pc = _path_call("class-paths" + ("-wide" if wide else ""), base, (0,), N, N)
    for rf in range(len(base.refs)):
        for w in CLASS_WIDTHS:
            a = int(rng.integers(0, CLASS_N - w + 1))
            pc.pair(0, rf, a, a + w)
    return pc


@functools.lru_cache(maxsize=None)
def class_paths_expected():
    pc = class_paths()
    query, valid, ref, ref_len = pc.call.arrays()
    return _frozen(*P.paths(query, valid, pc.call.quant, ref, ref_len, pc.pairs, pc.max_width))


# E. stretched copies: a path that stays on one reference row for 1 024 / C + 24 columns
STRETCH_N, STRETCH_WIDE_N, STRETCH_STRIDE, STRETCH_BG = 1728, 8192, 2048, 5
STRETCH_M = (40, 100, 200, 400, 800, 1600)


def stretch_length(c):
    return 1024 // c + 24


@functools.lru_cache(maxsize=None)
def stretched(wide=False):
    """(PathCall, [(i0, L)] per pair).  Pair p is read p against reference p over [0, the copy's end): the query is STRETCH_BG samples of
    background (90 and above; the references stay inside +-40 with no level twice in a row), the reference with its level i0 repeated L
    times, background.  Its only path at cost 0 holds L columns on row i0 and one on every other row"""
    rng = np.random.default_rng(5350)
    base = M.Call("stretched", STRETCH_N, 1.0, STRETCH_STRIDE)
    plan = []   # (M, i0)
    for m in STRETCH_M:
        c = rows_per_lane(m)
        lanes = (m - 1) // c + 1
        first = c * int(rng.integers(1, lanes))              # the first row of a lane
        last = c * int(rng.integers(1, lanes - 1)) + c - 1   # the last row of a lane (not of the last lane: its rows may end early)
        plan += [(m, first)] if c == 1 else [(m, first), (m, last)]
    plan += [(1, 0), (64, 63)]   # the sit on row 0; the last lane of C = 1
    ends, what = [], []
    for m, i0 in plan:
        L = stretch_length(rows_per_lane(m))
        ref = S._distinct(rng, -40, 40, m)
        copy = np.concatenate([ref[:i0], np.full(L, ref[i0]), ref[i0 + 1 :]])
        bg = rng.integers(90, 128, STRETCH_BG + len(copy) + 3)
        base.read(S._plant(bg, STRETCH_BG, copy))
        base.ref(ref)
        ends.append(STRETCH_BG + len(copy))
        what.append((i0, L))
    _fill(base, 5351)
    N = STRETCH_WIDE_N if wide else STRETCH_N
    pc = _path_call("stretched" + ("-wide" if wide else ""), base, tuple(range(len(plan))), N, N)
    for p, b in enumerate(ends):
        pc.pair(p, p, 0, b)
    return pc, tuple(what)


@functools.lru_cache(maxsize=None)
def stretched_expected():
    pc, _ = stretched()
    query, valid, ref, ref_len = pc.call.arrays()
    return _frozen(*P.paths(query, valid, pc.call.quant, ref, ref_len, pc.pairs, pc.max_width))


# F. the packed key's bound: the largest packed ref_stride of every sb, the cost field and the start field full at once
BOUND = ((4096, 2048), (8192, 1024), (16384, 512), (32768, 256), (65536, 128))


def bound_wide(N, stride):
    """the wide twin of a BOUND shape: ref_stride + 16, or -- ref_stride 2 048 is the header's largest -- query_len + 8"""
    return (N, stride + 16) if stride + 16 <= 2048 else (N + 8, stride)


@functools.lru_cache(maxsize=None)
def bound(index):
    """one reference of `stride` levels -128 against one read of N samples, all 127 but the last, 126: the straight walk down the last
    column costs 254 a row and is the only path at that cost, so (cost, end, start) = (254 stride, N, N - 1) -- and the keys beside the
    answer hold 255 (i + 1) with starts up to N - 2"""
    N, stride = BOUND[index]
    f = M.Call("bound-%d-%d" % (N, stride), N, 1.0, stride)
    q = np.full(N, 127)
    q[-1] = 126
    f.planted[(f.read(q), f.ref(np.full(stride, -128)))] = (254 * stride, N, N - 1)
    return f


@functools.lru_cache(maxsize=None)
def bound_spans(index):
    return _spans(bound(index))


@functools.lru_cache(maxsize=None)
def bound_paths(index):
    """(PathCall, (hit, rows)): the window [0, N) at max_width N"""
    f = bound(index)
    pc = _path_call(f.name, f, (0,), f.N, f.N)
    pc.pair(0, 0, 0, f.N)
    query, valid, ref, ref_len = pc.call.arrays()
    return pc, _frozen(*P.paths(query, valid, f.quant, ref, ref_len, pc.pairs, pc.max_width))


# G. consistency over A: the path call over (start, end) of every span
@functools.lru_cache(maxsize=None)
def dense_windows():
    """(PathCall over every pair of A with the window its span names, the hits it must write: uint32 [pairs, 4])"""
    a, spans = dense(), dense_spans()
    pc = _path_call("dense-windows", a, tuple(range(len(a.rows))), a.N, a.N)
    want = np.zeros((len(a.rows) * len(a.refs), 4), np.uint32)
    for rd in range(len(a.rows)):
        for rf in range(len(a.refs)):
            cost, end, start, _ = (int(v) for v in spans[rd][rf])
            want[pc.pair(rd, rf, start, end)] = (cost, end, start, a.ref_len[rf])
    return pc, _frozen(want)


# ---- 4. every launch of the sweep, as the census sees it --------------------------------------------------------------------------------------
def dense_shapes():
    """the launches of A, A-wide, C, C-wide and G: what the step residues of C = 1, 2, 4 are counted over"""
    a = dense()
    out = call_shapes(a) + [Shape("dense-wide", "span", DENSE_WIDE_N, DENSE_STRIDE, a.pairs())]
    return out + [path_shape(dense_paths()), path_shape(dense_paths_wide()), path_shape(dense_windows()[0])]


def sweep_shapes():
    out = dense_shapes()
    b = every()
    out += call_shapes(b) + [s.at("every-wide", N=EVERY_WIDE_N) for s in call_shapes(b)]
    out += [path_shape(class_paths()), path_shape(class_paths()).at("class-paths-wide", N=CLASS_WIDE_N)]
    out += [path_shape(stretched()[0]), path_shape(stretched()[0]).at("stretched-wide", N=STRETCH_WIDE_N)]
    for i, (N, stride) in enumerate(BOUND):
        f = bound(i)
        wN, ws = bound_wide(N, stride)
        out += [Shape(f.name, "span", N, stride, f.pairs()), Shape(f.name + "-wide", "span", wN, ws, f.pairs()), Shape(f.name, "path", N, stride, f.pairs())]
    return out


def sweep_long_runs():
    """long_runs of E and of its wide twin (the same pairs and rows under the other key)"""
    pc, _ = stretched()
    _, rows = stretched_expected()
    out = long_runs(pc, rows)
    wide, _ = stretched(True)
    out.update(long_runs(wide, rows))
    return out
