"""Reference for the path calls of the signal match (include/vbz_gpu.h: vbz_gpu_match_best_batch, vbz_gpu_match_path_batch), numpy and
python: the winners' table, the backtrace of one pair over its window, the enumeration of every path of a tiny pair, and the catalogue of
pairs the stage entry is held to on the device.  match_ref states quantisation and cost, match_span_ref the DP of pairs (cost, start).

The rule.  A pair is a read, a reference and a window [a, b) of the read's query.  Over the window's columns alone, P is
match_span_ref.span_matrix (row 0 at column a is (c(0, a), a): nothing left of a exists).  The path is the backtrace from (M - 1, b - 1):
at (i, j) with i > 0 and j > a it steps to the FIRST of diagonal, up, left whose P is the lexicographic minimum of the three; at j == a,
i > 0, up; in row 0 left while j > a and P[0][j-1].cost == 0, and stops otherwise.  Row i is aligned to samples [begin_i, end_i)."""
import functools

import numpy as np

import match_ref as M
import match_span_ref as S

EMPTY = (0xFFFFFFFF, 0, 0, 0)
NONE = 0xFFFFFFFF


def key_matrix(ref, k):
    """every row of keys cost << SHIFT | start of one pair, int64 [M, W], starts relative to the window (match_span_ref.span_rows,
    keeping the rows)"""
    K = np.asarray(k, np.int64)[None, :]
    rows, prev = [], None
    for r in np.asarray(ref, np.int64):
        c = np.abs(r - K)
        C = np.cumsum(c, axis=1)
        if prev is None:
            a = np.arange(K.shape[1], dtype=np.int64)[None, :].copy()
        else:
            a = prev.copy()
            a[:, 1:] = np.minimum(prev[:, 1:], prev[:, :-1])
        prev = (C << S.SHIFT) + np.minimum.accumulate(a - ((C - c) << S.SHIFT), axis=1)
        rows.append(prev[0])
    return np.stack(rows)


def matrix_keys(P):
    """match_span_ref.span_matrix's P as keys"""
    return np.array([[(c << S.SHIFT) | s for c, s in row] for row in P], np.int64)


def backtrace(K):
    """the cells of the rule's path through a matrix of keys, last cell first: [(i, j)]"""
    i, j = K.shape[0] - 1, K.shape[1] - 1
    cells = [(i, j)]
    while True:
        if i == 0:
            if j > 0 and (int(K[0][j - 1]) >> S.SHIFT) == 0:
                j -= 1
            else:
                return cells
        elif j == 0:
            i -= 1
        else:
            d, u, l = int(K[i - 1][j - 1]), int(K[i - 1][j]), int(K[i][j - 1])
            m = min(d, u, l)
            if d == m:
                i, j = i - 1, j - 1
            elif u == m:
                i -= 1
            else:
                j -= 1
        cells.append((i, j))


def path_pair(ref, k, a, b, brute=False):
    """(hit, rows) of one pair: hit = (cost, end, start, rows), rows int64 [M, 2] = (begin, end) per reference row.  ref: its M >= 1
    levels; k: the read's quantised query, 0 <= a < b <= len(k).  brute: P by match_span_ref.span_matrix's triple loop"""
    win = [int(v) for v in k[a:b]]
    K = matrix_keys(S.span_matrix(ref, win)) if brute else key_matrix(ref, win)
    cells = backtrace(K)
    rows = np.zeros((len(ref), 2), np.int64)
    rows[:, 0] = b
    for i, j in cells:
        rows[i][0] = min(rows[i][0], a + j)
        rows[i][1] = max(rows[i][1], a + j + 1)
    return (int(K[-1][-1]) >> S.SHIFT, b, a + cells[-1][1], len(ref)), rows


def all_paths(ref, k):
    """every warping path to (M - 1, n - 1) of a pair of at most 4 x 6, as (cost, start, cells last first); horizontal steps in row 0 count"""
    rows, n = len(ref), len(k)
    assert rows <= 4 and n <= 6
    c = [[abs(int(r) - int(q)) for q in k] for r in ref]
    out = []

    def walk(i, j, cost, cells):
        cost += c[i][j]
        cells = [(i, j)] + cells
        if i == rows - 1 and j == n - 1:
            out.append((cost, cells[-1][1], cells))
        if j + 1 < n:
            walk(i, j + 1, cost, cells)
            if i + 1 < rows:
                walk(i + 1, j + 1, cost, cells)
        if i + 1 < rows:
            walk(i + 1, j, cost, cells)

    for s in range(n):
        walk(0, s, 0, [])
    return out


def recost(ref, k, rows):
    """the sum of c(i, j) over the cells rows names: row i takes samples [begin_i, end_i)"""
    return sum(abs(int(r) - int(q)) for r, (b, e) in zip(ref, rows) for q in k[int(b) : int(e)])


def best(spans, max_cost=0xFFFFFFFF):
    """what the best launch writes: uint32 [reads, 4] = (read, ref, begin, end) from spans uint32 [reads, R, 4]"""
    out = np.zeros((len(spans), 4), np.uint32)
    for i, row in enumerate(spans):
        out[i] = (i, NONE, 0, 0)
        cand = [(int(h[0]), r) for r, h in enumerate(row) if int(h[0]) != EMPTY[0] and int(h[0]) <= max_cost]
        if cand:
            r = min(cand)[1]
            out[i] = (i, r, row[r][2], row[r][1])
    return out


def paths(query, valid, quant, ref, ref_len, pairs, max_width):
    """what a path call writes: (hit uint32 [pairs, 4], rows uint32 [pairs, ref_stride, 2]).  query float32 [reads, N] (valid None: N
    samples a row), ref int8 [R, ref_stride], pairs any integers [pairs, 4] = (read, ref, begin, end)"""
    N, stride = query.shape[1], ref.shape[1]
    hit = np.zeros((len(pairs), 4), np.uint32)
    rows = np.zeros((len(pairs), stride, 2), np.uint32)
    hit[:, 0] = EMPTY[0]
    K = {}
    for p, (rd, rf, a, b) in enumerate(np.asarray(pairs, np.uint64).tolist()):
        if rd >= len(query) or rf >= len(ref) or a >= b:
            continue
        n = N if valid is None else min(int(valid[rd]), N)
        m = int(ref_len[rf])
        if b > n or b - a > max_width or m == 0 or m > stride:
            continue
        if rd not in K:
            K[rd] = M.quantize(query[rd], quant)
        h, r = path_pair(ref[rf, :m], K[rd], a, b)
        hit[p] = h
        rows[p, :m] = r
    return hit, rows


# ---- the catalogue ------------------------------------------------------------------------------------------------------------------------
# A lane packs the directions of its c rows, step after step, into words of 16 cells: a word closes every 16 / c steps, and a lane's steps
# run from its own number on.  1 ... 129 as the issue lists them, and both sides of 16, 32, 48 and 64 steps (c = 1's word seams; c = 2's
# are at 8, 16, ..., and so on: every seam of every c up to 64 steps has a width on each side here or falls on one of these).
WIDTHS = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 129]


class PathCall:
    """one stage-entry call: a match_ref.Call (queries and references) with its pair table and max_width"""

    def __init__(self, name, N, quant, stride, max_width=None):
        self.call = M.Call(name, N, quant, stride)
        self.name, self.max_width, self.pairs = name, N if max_width is None else max_width, []

    def pair(self, read, ref, a, b):
        self.pairs.append((read, ref, a, b))
        return len(self.pairs) - 1


def _two_level(rng, n):
    return rng.integers(0, 2, n) * 3


@functools.lru_cache(maxsize=None)
def catalogue():
    rng = np.random.default_rng(4221)
    calls = []
    # every reference length against every width, windows at moving offsets of one read of signal
    c = PathCall("lengths", 256, 32.0, 2048, 136)
    rd = c.call.read(M._signal_levels(rng, 250))
    for m in M.LENGTHS_M:
        rf = c.call.ref(M._signal_levels(rng, m))
        for w in WIDTHS:
            a = int(rng.integers(0, 250 - w + 1))
            c.pair(rd, rf, a, a + w)
    calls.append(c)
    # two- and three-level alphabets with plateaus: all three predecessors tie
    c = PathCall("ties", 136, 1.0, 1040)
    reads = [c.call.read(_two_level(rng, 129)), c.call.read(rng.integers(-1, 2, 130)), c.call.read(np.repeat(rng.integers(-1, 2, 33), 4)[:129]),
             c.call.read(np.zeros(136))]
    refs = [c.call.ref(_two_level(rng, m) if m % 2 else rng.integers(-1, 2, m)) for m in S.TIE_M + S.TIE_SHORT] + [c.call.ref(np.zeros(70))]
    for rd in reads:
        for rf in refs:
            w = int(rng.choice(WIDTHS))
            a = int(rng.integers(0, 129 - w + 1))
            c.pair(rd, rf, a, a + w)
            c.pair(rd, rf, 0, 129)
    calls.append(c)
    # planted: sits on row 0 (whole and cut by a), M = 1, a = 0 and b = n, level -128
    c = PathCall("planted", 256, 1.0, 80)
    ref = S._distinct(rng, -40, 40, 17)
    rf, one, low = c.call.ref(ref), c.call.ref([7]), c.call.ref(np.full(5, -128))
    bg = rng.integers(90, 128, 256)
    run = c.call.read(S._plant(S._plant(bg, 100, ref), 95, np.full(5, ref[0])))   # the first level five times in front of the copy
    c.pair(run, rf, 80, 117)      # the sit behind a: start 95
    c.pair(run, rf, 97, 117)      # the sit cut by a: start 97
    c.pair(run, rf, 0, 256)       # a = 0 and b = n
    c.pair(run, rf, 0, 117)
    c.pair(run, rf, 100, 256)
    sevens = c.call.read(S._plant(bg, 200, np.full(9, 7)))
    c.pair(sevens, one, 190, 209)  # M = 1: sits on row 0 at cost 0 and stops at 200
    c.pair(sevens, one, 190, 220)  # ... the last column costs: no sit
    c.pair(sevens, one, 204, 205)  # W = 1, M = 1
    lo = c.call.read(np.full(40, -127))
    c.pair(lo, low, 3, 30)
    c.pair(lo, low, 7, 8)          # W = 1: all vertical
    c.pair(run, rf, 110, 111)
    calls.append(c)
    # one pair of 2 048 x 4 096
    c = PathCall("large", 4096, 32.0, 2048)
    c.pair(c.call.read(M._signal_levels(rng, 4096)), c.call.ref(M._signal_levels(rng, 2048)), 0, 4096)
    calls.append(c)
    # one data set on both sides of the packed / wide rule, max_width = N
    reads = [M._signal_levels(rng, 4096), rng.integers(-3, 4, 1000), rng.integers(-1, 2, 65), M._signal_levels(rng, 4095)]
    refs = [M._signal_levels(rng, 257), rng.integers(-3, 4, 129), rng.integers(-1, 2, 64), M._signal_levels(rng, 17)]
    windows = [(0, 4096), (13, 1000), (0, 65), (2000, 4095)]
    for N, stride in ((4096, 2048), (8192, 2048), (16384, 416), (32768, 416)):
        c = PathCall("rule-%d-%d" % (N, stride), N, 32.0, stride)
        for x in reads:
            c.call.read(x)
        for x in refs:
            c.call.ref(x)
        for rd, (a, b) in enumerate(windows):
            for rf in range(len(refs)):
                c.pair(rd, rf, a, b)
        calls.append(c)
    return calls


@functools.lru_cache(maxsize=None)
def expected(index):
    """(hit, rows) of catalogue()[index], computed once (the four rule calls share one computation: their data is one data set)"""
    calls = catalogue()
    c = calls[index]
    if c.name.startswith("rule-"):
        first = next(i for i, x in enumerate(calls) if x.name.startswith("rule-"))
        if index != first:
            hit, rows = expected(first)
            wide = np.zeros((len(rows), c.call.stride, 2), np.uint32)
            wide[:, : min(rows.shape[1], c.call.stride)] = rows[:, : c.call.stride]
            assert not rows[:, c.call.stride :].any()
            wide.setflags(write=False)
            return hit, wide
    query, valid, ref, ref_len = c.call.arrays()
    hit, rows = paths(query, valid, c.call.quant, ref, ref_len, c.pairs, c.max_width)
    hit.setflags(write=False)
    rows.setflags(write=False)
    return hit, rows
