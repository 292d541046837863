"""Reference for the signal-locate calls (include/vbz_gpu.h: vbz_gpu_locate), pure numpy, built on match_ref: the read's whole quantised
prefix aligned to a stretch of a long int8 target.  The statement is match_ref's with its arguments exchanged --

    locate(levels of the read, target[:L]) = match_ref.dtw_batch(levels, target[None, :L], [L])

-- rows the query, columns the target, the free start and the free end in the target.  The catalogue of calls the stage entry is held to on
the device lives here too."""
import functools

import numpy as np

import match_ref as M

EMPTY = M.EMPTY
LENGTHS_N = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048]
LENGTHS_L = [1, 2, 63, 64, 65, 255, 256, 257, 1000]
ROWS = (1, 2, 4, 8, 16, 32)


def rows_per_lane(n):
    """c: the smallest of 1, 2, 4, 8, 16, 32 with 64 c >= n"""
    return next(c for c in ROWS if 64 * c >= n)


def locate(levels, target):
    """(cost, end) of one pair: levels int [n] (the query, aligned whole), target int [L]"""
    if len(levels) == 0 or len(target) == 0:
        return EMPTY
    cost, end = M.dtw_batch(np.asarray(levels, np.int64), np.asarray(target, np.int64)[None, :], [len(target)])
    return int(cost[0]), int(end[0])


def hits(query, valid, quant, target, target_len):
    """what a locate launch writes: uint32 [reads, G, 2].  query float32 [reads, N]; target int8 [G, stride]; valid, target_len: any
    integers 0 ... 2^32 - 1.  (One walk per read over all its good target rows at once: a position only depends on positions in front of
    it, so what stands behind a row's end never reaches an answer.)"""
    N, stride = query.shape[1], target.shape[1]
    K = M.quantize(query, quant)
    n = np.minimum(np.asarray(valid, np.uint64), N).astype(np.int64)
    L = np.asarray(target_len, np.uint64)
    good = np.flatnonzero((L != 0) & (L <= stride))
    out = np.zeros((len(query), len(target), 2), np.uint32)
    out[:, :, 0] = EMPTY[0]
    if good.size == 0:
        return out
    T = np.asarray(target, np.int64)[good]
    Lg = L[good].astype(np.int64)
    T = T[:, : int(Lg.max())]
    for i in range(len(query)):
        if n[i] == 0:
            continue
        out[i, good, 0], out[i, good, 1] = M.dtw_batch(K[i, : n[i]], T, Lg)
    return out


# ---- the catalogue ------------------------------------------------------------------------------------------------------------------------
class Call:
    """one stage-entry call: queries (float32 [reads, N]) with their valid counts against target rows (int8 [G, stride]) with their lengths;
    planted: {(read, target): (cost, end)} known without running the DP.  What stands behind a target's end is random int8, never 0 alone."""

    def __init__(self, name, N, quant, stride, seed):
        self.name, self.N, self.quant, self.stride = name, N, quant, stride
        self.rng = np.random.default_rng(seed)
        self.rows, self.valid, self.targets, self.target_len, self.planted = [], [], [], [], {}

    def read(self, levels=None, z=None, valid=None):
        """a query row from int levels (z = level / quant: exact for a power-of-two quant) or from floats as they are"""
        row = np.zeros(self.N, np.float32)
        if z is None:
            z = np.asarray(levels, np.float32) / np.float32(self.quant)
        row[: len(z)] = z
        self.rows.append(row)
        self.valid.append(len(z) if valid is None else valid)
        return len(self.rows) - 1

    def target(self, levels, length=None):
        row = self.rng.integers(-128, 128, self.stride).astype(np.int8)
        row[row == 0] = -128
        row[: len(levels)] = levels
        self.targets.append(row)
        self.target_len.append(len(levels) if length is None else length)
        return len(self.targets) - 1

    def arrays(self):
        return (np.stack(self.rows), np.asarray(self.valid, np.uint64).astype(np.uint32), np.stack(self.targets),
                np.asarray(self.target_len, np.uint64).astype(np.uint32))

    def pairs(self):
        """(n, L) of every pair that runs the DP"""
        return [(min(int(v), self.N), int(L)) for v in self.valid for L in self.target_len if 0 < int(L) <= self.stride and int(v) != 0]


def signal_levels(rng, n, lowest=False):
    """levels like MAD-normalised signal at 32 a unit: plateaus under noise; lowest: a target's, with -128 among them"""
    steps = np.repeat(rng.integers(-70, 71, n // 6 + 1), 6)[:n]
    x = np.clip(steps + rng.integers(-6, 7, n), -127, 127)
    if lowest and n:
        x[rng.integers(0, n, n // 9 + 1)] = -128
    return x


def distinct_levels(rng, n):
    """levels inside +-40 with no level twice in a row: no alignment at cost 0 ends in front of a copy's end"""
    q = rng.integers(-40, 41, n)
    for i in range(1, n):
        if q[i] == q[i - 1]:
            q[i] += 1 if q[i] < 40 else -1
    return q


def plant(bg, at, what):
    t = np.array(bg, np.int64)
    assert 0 <= at and at + len(what) <= len(t), (at, len(what), len(t))
    t[at : at + len(what)] = what
    return t


LONG_L, LONG_END = 70_000, 66_142


@functools.lru_cache(maxsize=None)
def catalogue():
    """the calls of tests/test_gpu_locate.py: every n of LENGTHS_N against every L of LENGTHS_L, valid above N, refused target_len beside
    good rows, the planted answers, the extremes, and one long target that no match call can express"""
    calls = []
    a = Call("lengths", 2048, 32.0, 1008, 2310)
    for n in LENGTHS_N:
        a.read(signal_levels(a.rng, n))
    a.read(signal_levels(a.rng, 2048), valid=5000)        # valid above N is clamped to N
    a.read(signal_levels(a.rng, 2048), valid=0xFFFFFFFF)
    for L in LENGTHS_L:
        a.target(signal_levels(a.rng, L, lowest=True))
    a.target(signal_levels(a.rng, 40), length=0)           # refused lengths beside good ones
    a.target(signal_levels(a.rng, 40), length=1009)
    a.target(signal_levels(a.rng, 40), length=0xFFFFFFFF)
    a.target(signal_levels(a.rng, 100, lowest=True))
    calls.append(a)
    # planted answers: cost 0 and a known end.  The query's levels stay inside +-40, the background at 90 and above.  Blocks of the
    # loader: 64 dwords = 256 levels
    p = Call("planted", 640, 32.0, 2048, 2311)
    for n in (17, 129, 600):
        q = distinct_levels(p.rng, n)
        ri = p.read(q)
        L = 2048
        bg = p.rng.integers(90, 128, L)
        for at in (0, L - n, 256 - n // 2 if n < 512 else 512 - n // 2):   # its very start, its very end, across a block seam
            p.planted[(ri, p.target(plant(bg, at, q)))] = (0, at + n)
        p.planted[(ri, p.target(plant(bg, 30, np.repeat(q, 3))))] = (0, 30 + 3 * n - 2)    # every level tripled: the first-j rule
        p.planted[(ri, p.target(plant(plant(bg, 10, q), 1100, q)))] = (0, 10 + n)           # two equal plants: the first
    calls.append(p)
    # extremes
    e = Call("extremes", 64, 1.0, 304, 2312)
    lo, hi = e.target(np.full(300, -128)), e.target(np.full(304, 127))
    e.target(e.rng.integers(-128, 128, 200))
    e.target(e.rng.integers(-128, 128, 64))
    e.target(np.full(1, -128))
    q_hi, q_lo = e.read(np.full(64, 127)), e.read(np.full(9, -127))
    e.read(e.rng.integers(-127, 128, 64))
    e.read(e.rng.integers(-127, 128, 33))
    e.planted[(q_hi, lo)] = (255 * 64, 1)
    e.planted[(q_lo, lo)] = (1 * 9, 1)
    e.planted[(q_lo, hi)] = (254 * 9, 1)
    # the quantisation inside a call: match_ref's "extremes" row -- ties of both parities, the clamp, NaN, infinities
    e.read(z=np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5, 127.5, 200.0, -127.5, -1e30, np.nan, np.inf, -np.inf, 3e38, 0.49999997], np.float32))
    calls.append(e)
    f = Call("floats", 208, 10.3, 400, 2313)
    for n in (200, 77):
        f.read(z=f.rng.normal(0, 4, n).astype(np.float32))
    for L in (5, 333, 400):
        f.target(M.quantize(f.rng.normal(0, 4, L), 10.3))
    calls.append(f)
    # one long call: L beyond 65 536, which no match call can express with the roles swapped
    g = Call("long", 2048, 32.0, 70_016, 2314)
    g.read(signal_levels(g.rng, 2048))
    q = distinct_levels(g.rng, 700)
    short = g.read(q)
    bg = g.rng.integers(90, 128, LONG_L)
    g.planted[(short, g.target(plant(bg, LONG_END + 2 - 3 * 700, np.repeat(q, 3))))] = (0, LONG_END)   # tripled, ending beyond 65 536
    calls.append(g)
    return calls


@functools.lru_cache(maxsize=None)
def expected(index):
    """the hits of catalogue()[index], computed once"""
    c = catalogue()[index]
    query, valid, target, target_len = c.arrays()
    out = hits(query, valid, c.quant, target, target_len)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def sweep(top=136, stride=144):
    """the dense sweep: every n = 1 ... top against every L = 1 ... top.  NaN, infinities and +-1e30 behind every read's end; random int8,
    -128 among them, behind every target's end -> (query float32 [top, top], valid, target int8 [top, stride], target_len, hits)"""
    rng = np.random.default_rng(2315)
    junk = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32)
    query = junk[rng.integers(0, len(junk), (top, top))]
    target = rng.integers(-128, 128, (top, stride)).astype(np.int8)
    target[:, top:][target[:, top:] == 0] = -128
    for i in range(top):
        n = i + 1
        query[i, :n] = signal_levels(rng, n).astype(np.float32) / np.float32(32.0)
        target[i, :n] = signal_levels(rng, n, lowest=True)
    lens = np.arange(1, top + 1, dtype=np.uint32)
    want = hits(query, lens, 32.0, target, lens)
    for a in (query, target, want):
        a.setflags(write=False)
    return query, lens, target, lens, want
