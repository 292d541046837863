"""Reference for the path call of the signal locate (include/vbz_gpu.h: vbz_gpu_locate_path_batch) and for vbz_gpu_query_valid_batch, numpy
and python.  The rule is the match-path rule with its arguments exchanged --

    path(levels of the read[:n], target[:L], a, b) = match_path_ref.path_pair(levels, target[:L], a, b)

-- rows the query, columns the target, [a, b) a window of TARGET levels.  paths() applies the pair rules of the header on top of it; it
computes the keys of the pairs of one read in one walk down the query (a window's columns only depend on columns to their left, so
windows of different widths share a zero-padded matrix), and test_locate_path_ref holds that to the statement.  The catalogue of calls the
stage entry is held to on the device lives here too."""
import functools

import numpy as np

import locate_ref as LR
import match_path_ref as P
import match_ref as M
import match_span_ref as S

EMPTY = P.EMPTY
NONE = P.NONE
WIDTHS = P.WIDTHS
E_FIRST = 0xFFFFFFF8   # verdicts from here on are errors (_lib.VBZ_DEVICE_ERROR)


def path_pair(levels, target, a, b, brute=False):
    """the statement: (hit, rows) of one pair, hit = (cost, b, start, n), rows int64 [n, 2] = (begin, end) in target coordinates"""
    return P.path_pair(levels, target, a, b, brute=brute)


def key_windows(levels, windows):
    """the keys cost << SHIFT | start of one query against several windows at once: windows int [B, Wmax] (zero-padded behind a window's
    width) -> int64 [n, B, Wmax], starts relative to each window (match_path_ref.key_matrix over a batch of columns)"""
    K = np.asarray(windows, np.int64)
    rows, prev = [], None
    for r in np.asarray(levels, np.int64):
        c = np.abs(r - K)
        C = np.cumsum(c, axis=1)
        if prev is None:
            a = np.broadcast_to(np.arange(K.shape[1], dtype=np.int64), K.shape).copy()
        else:
            a = prev.copy()
            a[:, 1:] = np.minimum(prev[:, 1:], prev[:, :-1])
        prev = (C << S.SHIFT) + np.minimum.accumulate(a - ((C - c) << S.SHIFT), axis=1)
        rows.append(prev)
    return np.stack(rows)


def _trace(K, a, b, n):
    cells = P.backtrace(K)
    rows = np.zeros((n, 2), np.int64)
    rows[:, 0] = b
    for i, j in cells:
        rows[i][0] = min(rows[i][0], a + j)
        rows[i][1] = max(rows[i][1], a + j + 1)
    return (int(K[-1][-1]) >> S.SHIFT, b, a + cells[-1][1], n), rows


def paths(query, valid, quant, target, target_len, pairs, max_width):
    """what a locate path call writes: (hit uint32 [pairs, 4], rows uint32 [pairs, N, 2]).  query float32 [reads, N], valid any integers
    [reads], target int8 [G, stride], pairs any integers [pairs, 4] = (read, target, begin, end)"""
    N, stride = query.shape[1], target.shape[1]
    hit = np.zeros((len(pairs), 4), np.uint32)
    rows = np.zeros((len(pairs), N, 2), np.uint32)
    hit[:, 0] = EMPTY[0]
    by_read = {}
    for p, (rd, tg, a, b) in enumerate(np.asarray(pairs, np.uint64).reshape(-1, 4).tolist()):
        if rd >= len(query) or tg >= len(target) or a >= b:
            continue
        n = min(int(valid[rd]), N)
        L = int(target_len[tg])
        if n == 0 or L == 0 or L > stride or b > L or b - a > max_width:
            continue
        by_read.setdefault(rd, []).append((b - a, p, tg, a, b))
    for rd, todo in by_read.items():
        n = min(int(valid[rd]), N)
        levels = M.quantize(query[rd], quant)[:n]
        todo.sort()
        at = 0
        while at < len(todo):   # groups of similar widths, a bounded matrix each
            group = [todo[at]]
            while at + len(group) < len(todo) and len(group) < 32 and n * (len(group) + 1) * todo[at + len(group)][0] <= 1 << 24:
                group.append(todo[at + len(group)])
            at += len(group)
            win = np.zeros((len(group), group[-1][0]), np.int64)
            for g, (w, p, tg, a, b) in enumerate(group):
                win[g, :w] = target[tg, a:b]
            K = key_windows(levels, win)
            for g, (w, p, tg, a, b) in enumerate(group):
                hit[p], rows[p, :n] = _trace(K[:, g, :w], a, b, n)
    return hit, rows


def query_valid(result, query_len, begin=None, end=None):
    """what vbz_gpu_query_valid_batch writes: min(T', N) of a read whose verdict is T x 4 bytes, its range clamped as sample_range clamps
    it; 0 for an error verdict"""
    out = np.zeros(len(result), np.uint32)
    for i, res in enumerate(np.asarray(result, np.uint64).tolist()):
        if res >= E_FIRST:
            continue
        T = res // 4
        e = T if end is None else min(int(end[i]), T)
        b = 0 if begin is None else min(int(begin[i]), e)
        out[i] = min(e - b, query_len)
    return out


# ---- the catalogue ------------------------------------------------------------------------------------------------------------------------
ROWS_SMALL = list(range(1, 137))
ROWS_LARGE = [255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048]   # both sides of every change of the rows per lane


class PathCall:
    """one stage-entry call: a locate_ref.Call (queries and targets) with its pair table and max_width; planted: {pair: (hit, rows or
    None)} known without the DP"""

    def __init__(self, name, N, quant, stride, seed, max_width):
        self.call = LR.Call(name, N, quant, stride, seed)
        self.name, self.max_width, self.pairs, self.planted, self.rng = name, max_width, [], {}, self.call.rng

    def pair(self, read, target, a, b):
        self.pairs.append((read, target, a, b))
        return len(self.pairs) - 1


def _two_level(rng, n):
    return rng.integers(0, 2, n) * 3


def _rows(name, lengths, seed):
    """every n of `lengths` against windows of every width of WIDTHS at moving offsets of one target of signal"""
    N = (max(lengths) + 7) // 8 * 8
    c = PathCall(name, N, 32.0, 1008, seed, 136)
    tg = c.call.target(LR.signal_levels(c.rng, 1003, lowest=True))
    for n in lengths:
        rd = c.call.read(LR.signal_levels(c.rng, n))
        for w in WIDTHS:
            a = int(c.rng.integers(0, 1003 - w + 1))
            c.pair(rd, tg, a, a + w)
    return c


def _bytes():
    """the byte stream: one call a part.  Target 0 has L = 1003 levels (L % 4 == 3) in a row of 1008, target 1 the same levels with other
    junk behind them"""
    out = []

    def call(name, max_width=520):
        c = PathCall("bytes-" + name, 136, 32.0, 1008, 4302, max_width)
        levels = LR.signal_levels(c.rng, 1003, lowest=True)
        c.call.target(levels)
        c.call.target(levels)
        assert (c.call.targets[0][1003:] != c.call.targets[1][1003:]).any()
        c.call.read(LR.signal_levels(c.rng, 17))
        c.call.read(LR.signal_levels(c.rng, 129))
        out.append(c)
        return c

    c = call("residues")
    for rd in (0, 1):
        for ra in range(4):
            for rb in range(4):
                a = 40 + 4 * int(c.rng.integers(0, 100)) + ra
                b = a + 36 + (rb - a) % 4
                assert a % 4 == ra and b % 4 == rb
                c.pair(rd, 0, a, b)
                c.pair(rd, 0, a, a + 1 + (rb - a - 1) % 4)   # inside one dword, or just across its end
    c = call("a0")
    for rd in (0, 1):
        for b in (1, 2, 3, 4, 5, 64, 255, 256, 257, 520):
            c.pair(rd, 0, 0, b)
    c = call("bL")
    for rd in (0, 1):
        for a in (1002, 1001, 1000, 999, 998, 900, 747, 746, 745, 483):
            c.pair(rd, 0, a, 1003)
    c = call("junk")
    for rd in (0, 1):
        for a in (1002, 1000, 997, 870, 483):
            c.pair(rd, 0, a, 1003)
            c.pair(rd, 1, a, 1003)   # the same levels, other bytes behind them: the same answer
    c = call("blocks")
    for rd in (0, 1):
        for w in (255, 256, 257, 511, 512, 513):
            for ra in range(4):
                a = 4 * int(c.rng.integers(0, 100)) + ra
                c.pair(rd, 0, a, a + w)
    return out


def _ties():
    c = PathCall("ties", 136, 1.0, 304, 4303, 304)
    reads = [c.call.read(_two_level(c.rng, n)) for n in (3, 9, 63, 64, 65, 129)]
    reads += [c.call.read(np.repeat(c.rng.integers(-1, 2, 33), 4)[:129]), c.call.read(np.zeros(136)), c.call.read(c.rng.integers(-1, 2, 130))]
    targets = [c.call.target(_two_level(c.rng, 301)), c.call.target(np.repeat(_two_level(c.rng, 76), 4)[:302]), c.call.target(np.zeros(300)),
               c.call.target(c.rng.integers(-1, 2, 303))]
    for rd in reads:
        for tg in targets:
            w = int(c.rng.choice(WIDTHS))
            a = int(c.rng.integers(0, 300 - w + 1))
            c.pair(rd, tg, a, a + w)
            c.pair(rd, tg, 0, 300)
    return c


def _planted():
    """a run of the query's first level in front of a plant: touching it, not touching it, reaching a; the answers known without the DP"""
    c = PathCall("planted", 64, 32.0, 2048, 4304, 520)
    q = LR.distinct_levels(c.rng, 17)
    rd = c.call.read(q)
    bg = c.rng.integers(90, 128, 2048)
    exact = [[700 + i, 701 + i] for i in range(17)]
    touching = c.call.target(LR.plant(LR.plant(bg, 700, q), 695, np.full(5, q[0])))
    apart = c.call.target(LR.plant(LR.plant(bg, 700, q), 694, np.full(5, q[0])))   # one level of background between run and plant
    sat = [[695, 701]] + exact[1:]
    c.planted[c.pair(rd, touching, 650, 717)] = ((0, 717, 695, 17), sat)                       # the sit whole: start at the run's first level
    c.planted[c.pair(rd, touching, 697, 717)] = ((0, 717, 697, 17), [[697, 701]] + exact[1:])   # the sit cut by the window: it reaches a
    c.planted[c.pair(rd, touching, 695, 717)] = ((0, 717, 695, 17), sat)                       # ... a at the run's first level
    c.planted[c.pair(rd, touching, 700, 717)] = ((0, 717, 700, 17), exact)
    c.planted[c.pair(rd, apart, 650, 717)] = ((0, 717, 700, 17), exact)                        # not touching: the start does not move
    c.planted[c.pair(rd, apart, 200, 717)] = ((0, 717, 700, 17), exact)
    one = c.call.read([7])
    sevens = c.call.target(LR.plant(bg, 200, np.full(9, 7)))
    c.planted[c.pair(one, sevens, 190, 209)] = ((0, 209, 200, 1), [[200, 209]])   # n = 1: the path sits on row 0 at cost 0
    c.planted[c.pair(one, sevens, 204, 205)] = ((0, 205, 204, 1), [[204, 205]])   # W = 1, n = 1
    c.pair(one, sevens, 190, 220)                                                  # the last column costs: no sit
    c.pair(rd, touching, 710, 711)                                                 # W = 1: all vertical
    return c


def _lowest():
    """target levels of -128"""
    c = PathCall("lowest", 72, 1.0, 304, 4305, 304)
    lo, mixed = c.call.target(np.full(299, -128)), c.call.target(LR.signal_levels(c.rng, 301, lowest=True))
    reads = [c.call.read(np.full(40, -127)), c.call.read(np.full(9, 127)), c.call.read(c.rng.integers(-127, 128, 65)), c.call.read(np.full(5, -127))]
    for rd in reads:
        for tg in (lo, mixed):
            c.pair(rd, tg, 3, 30)
            c.pair(rd, tg, 7, 8)
            c.pair(rd, tg, 0, 299)
    c.planted[3 * 6] = ((5, 30, 25, 5), [[25 + i, 26 + i] for i in range(5)])   # five levels of -127 on -128: every cell costs 1, the diagonal starts first
    return c


KEY_WIDTHS = (4096, 4104)   # query_len 2 048: the packed key and the wide one (csrc/match_select.h with max_width in N's place)


def _keys(max_width):
    """one data set on both sides of the packed / wide rule; its first pair is 2 048 x 4 096"""
    c = PathCall("keys-%d" % max_width, 2048, 32.0, 4112, 4306, max_width)
    tg = c.call.target(LR.signal_levels(c.rng, 4101, lowest=True))
    small = c.call.target(c.rng.integers(-3, 4, 1000))
    c.pair(c.call.read(LR.signal_levels(c.rng, 2048)), tg, 0, 4096)
    c.pair(c.call.read(LR.signal_levels(c.rng, 257)), tg, 5, 4101)
    c.pair(c.call.read(c.rng.integers(-3, 4, 129)), small, 13, 1000)
    c.pair(c.call.read(c.rng.integers(-1, 2, 64)), small, 0, 65)
    return c


BEYOND_A = 65_538


def _beyond():
    """a window with a > 65 536 in locate_ref's long target: the last 200 levels of its tripled plant as the query"""
    long = LR.catalogue()[-1]
    assert long.name == "long" and long.stride == 70_016
    c = PathCall("beyond", 208, 32.0, 70_016, 4307, 608)
    c.call.targets.append(long.targets[0])
    c.call.target_len.append(long.target_len[0])
    q = M.quantize(long.rows[1], 32.0)[:700]
    at = LR.LONG_END + 2 - 3 * 700 + 3 * 500   # where level 500's three copies begin
    assert at > BEYOND_A > 65_536
    rd = c.call.read(q[500:])
    rows = [[at + 3 * i, at + 3 * i + 3] for i in range(199)] + [[LR.LONG_END - 1, LR.LONG_END]]
    c.planted[c.pair(rd, 0, BEYOND_A, LR.LONG_END)] = ((0, LR.LONG_END, at, 200), rows)
    return c


@functools.lru_cache(maxsize=None)
def catalogue():
    return [_rows("rows-small", ROWS_SMALL, 4300), _rows("rows-large", ROWS_LARGE, 4301)] + _bytes() + [_ties(), _planted(), _lowest()] + \
           [_keys(w) for w in KEY_WIDTHS] + [_beyond()]


@functools.lru_cache(maxsize=None)
def expected(index):
    """(hit, rows) of catalogue()[index], computed once (the two key calls share one computation: their data is one data set)"""
    calls = catalogue()
    c = calls[index]
    first = next(i for i, x in enumerate(calls) if x.name.startswith("keys-"))
    if c.name.startswith("keys-") and index != first:
        assert c.pairs == calls[first].pairs
        return expected(first)
    query, valid, target, target_len = c.call.arrays()
    hit, rows = paths(query, valid, c.call.quant, target, target_len, c.pairs, c.max_width)
    hit.setflags(write=False)
    rows.setflags(write=False)
    return hit, rows
