"""Reference for the signal-locate calls that also give the start of the aligned stretch (include/vbz_gpu.h: vbz_gpu_locate_span_batch),
pure numpy, built on locate_ref and match_span_ref.  The rule is the match-span rule with its arguments exchanged --

    span(levels of the read, target[:L]) = match_span_ref.span_brute(levels, target[:L])

-- rows the query, columns the target.  Three statements of it live here:

  the row form      match_span_ref's, over int64 keys cost << 32 | start (a start may need 30 bits: a shift of its own);
  the walk back     the reversed ANCHORED DP from the known (cost, end): D'[i'][j'] is the least cost of a path from cell
                    (n - 1 - i', end - 1 - j') to (n - 1, end - 1), and start = end - 1 - (the largest j' with D'[n - 1][j'] == cost).
                    Column minima of D' never decrease, so the walk may stop at the first column that exceeds cost as a whole;
  the front rule    a model of the device's stopping test: lane l of a systolic wavefront of c rows a lane is at column t - l at step
                    t; once every live cell of the fronts of two consecutive steps exceeds cost, no later step holds cost.
                    steps_back counts the steps of the device's walk by that rule, and wavefront_back restates the kernel lane by lane.

The catalogue of calls the stage entry is held to on the device lives here too."""
import functools

import numpy as np

import locate_ref as LR
import match_ref as M

EMPTY = (0xFFFFFFFF, 0, 0, 0)
SHIFT = 32
FAR = np.int64(1) << 60


# ---- the row form -------------------------------------------------------------------------------------------------------------------------
def span_rows(levels, T):
    """the last row of keys cost << 32 | start of the query `levels` (int [n], n >= 1) against every row of T (int [G, L]), int64 [G, L]"""
    T = np.asarray(T, np.int64)
    prev = None
    for k in np.asarray(levels, np.int64):
        c = np.abs(k - T)
        C = np.cumsum(c, axis=1)
        if prev is None:
            a = np.broadcast_to(np.arange(T.shape[1], dtype=np.int64), T.shape).copy()
        else:
            a = prev.copy()
            a[:, 1:] = np.minimum(prev[:, 1:], prev[:, :-1])
        prev = (C << SHIFT) + np.minimum.accumulate(a - ((C - c) << SHIFT), axis=1)
    return prev


def span_batch(levels, T, L):
    """(cost, end, start) uint32 [G] each of one query against target rows T[g, :L[g]] (every L[g] >= 1, len(levels) >= 1)"""
    last = span_rows(levels, T)
    last[np.arange(T.shape[1])[None, :] >= np.asarray(L, np.int64)[:, None]] = FAR
    best = last.min(axis=1)
    return (best >> SHIFT).astype(np.uint32), (last.argmin(axis=1) + 1).astype(np.uint32), (best & ((1 << SHIFT) - 1)).astype(np.uint32)


def span(levels, target):
    """(cost, end, start) of one pair"""
    if len(levels) == 0 or len(target) == 0:
        return EMPTY[:3]
    cost, end, start = span_batch(levels, np.asarray(target, np.int64)[None, :], [len(target)])
    return int(cost[0]), int(end[0]), int(start[0])


def spans(query, valid, quant, target, target_len):
    """what a locate span launch writes: uint32 [reads, G, 4] = (cost, end, start, 0).  Arguments as locate_ref.hits"""
    N, stride = query.shape[1], target.shape[1]
    K = M.quantize(query, quant)
    n = np.minimum(np.asarray(valid, np.uint64), N).astype(np.int64)
    L = np.asarray(target_len, np.uint64)
    good = np.flatnonzero((L != 0) & (L <= stride))
    out = np.zeros((len(query), len(target), 4), np.uint32)
    out[:, :, 0] = EMPTY[0]
    if good.size == 0:
        return out
    Lg = L[good].astype(np.int64)
    T = np.asarray(target, np.int64)[good][:, : int(Lg.max())]
    for i in range(len(query)):
        if n[i] == 0:
            continue
        out[i, good, 0], out[i, good, 1], out[i, good, 2] = span_batch(K[i, : n[i]], T, Lg)
    return out


# ---- the walk back ------------------------------------------------------------------------------------------------------------------------
def back_matrix(levels, target, end):
    """D' int64 [n, end] of the reversed anchored DP: D'[-1][-1] = 0, every other D'[-1][.] and D'[.][-1] far"""
    k = np.asarray(levels, np.int64)[::-1]
    g = np.asarray(target, np.int64)[:end][::-1]
    prev = np.full(end + 1, FAR, np.int64)   # row -1, with column -1 in front
    prev[0] = 0
    D = np.empty((len(k), end), np.int64)
    for i, ki in enumerate(k):
        c = np.abs(ki - g)
        C = np.cumsum(c)
        a = np.minimum(prev[1:], prev[:-1])
        D[i] = C + np.minimum.accumulate(a - (C - c))
        prev = np.concatenate(([FAR], D[i]))
    return D


def walk_back(levels, target, cost, end):
    """(start, columns walked): the start by the reversed statement, reading D' no further than the first column whose minimum exceeds
    cost (all of it when there is none)"""
    D = back_matrix(levels, target, end)
    over = np.flatnonzero(D.min(axis=0) > cost)
    stop = int(over[0]) if over.size else end
    held = np.flatnonzero(D[-1, :stop] == cost)
    assert held.size, "the known cost is not in the tracked row"
    return end - 1 - int(held[-1]), stop


def front_stop(D, cost, c):
    """the model of the device's rule over D' = back_matrix(...), c rows a lane: (the first step t + 1 such that every live cell -- a row
    of the query, a column met and inside the target -- of the fronts of steps t and t + 1 exceeds cost, or None; the step at which the
    last cell of the tracked row that holds cost is computed)"""
    n, end = D.shape
    lane = np.arange(n) // c
    la = (n - 1) // c
    last = int(np.flatnonzero(D[-1] == cost)[-1]) + la
    rows = np.arange(n)
    before = False
    for t in range(end + la):
        col = t - lane
        live = (col >= 0) & (col < end)
        over = not live.any() or int(D[rows[live], col[live]].min()) > cost
        if over and before:
            return t, last
        before = over
    return None, last


def steps_back(levels, target, cost, end, start, c):
    """the steps the device's walk back of one pair takes, c rows a lane: it tests the rule once a block of 256 virtual steps (virtual
    step v = t + skip, skip = 3 - (end - 1) % 4: the stream's dwords), on the fronts of the block's last two steps, and ends behind the
    first block that passes, or at the target's first level (end + la steps).  D' is computed over as many columns as that needs"""
    n = len(levels)
    la = (n - 1) // c
    skip = 3 - (end - 1) % 4
    lane = np.arange(n) // c
    rows = np.arange(n)
    W = min(end, end - start + 4096)
    while True:
        D = back_matrix(levels, target[end - W : end], W)
        v = 255
        while v - skip < min(W, end) + la - 1:
            over = True
            for t in (v - 1 - skip, v - skip):
                col = t - lane
                live = (col >= 0) & (col < W)
                over = over and (not live.any() or int(D[rows[live], col[live]].min()) > cost)
            if over and v - skip - la >= end - 1 - start:
                return v + 1 - skip
            v += 256
        if W == end:
            return end + la
        W = min(end, 2 * W)


def _msad(g, k, acc):
    """v_msad_u8: acc + the sum of |g_b - k_b| over the four bytes b where k_b != 0"""
    out = acc.copy()
    for b in range(4):
        gb, kb = (g >> (8 * b)) & 0xFF, (k >> (8 * b)) & 0xFF
        out += np.where(kb != 0, np.abs(gb - kb), 0)
    return out


def wavefront_back(levels, target, cost, end, c):
    """the device's walk back (csrc/locate.hip: locate_back) restated lane by lane over 64-entry int64 vectors: the reversed query as words
    k + 128 with 0x100 in the rows behind n, the stream as byte-swapped dwords from level end - 1 down, the anchored start, the selects of
    row (n - 1) mod c, the fronts of a block's last two steps, the clamp -> (start, steps taken)"""
    far = 1 << 30
    levels = np.asarray(levels, np.int64)
    n = len(levels)
    lane = np.arange(64)
    la, track = (n - 1) // c, (n - 1) % c
    padded = np.zeros((len(target) + 3) // 4 * 4, np.uint8)
    padded[: len(target)] = np.asarray(target, np.int64).astype(np.int8).view(np.uint8)
    words = padded.view("<u4").astype(np.int64)
    k = np.empty((c, 64), np.int64)
    for i in range(c):
        r = lane * c + i
        k[i] = np.where(r < n, levels[np.clip(n - 1 - r, 0, n - 1)] + 128, 0x100)
    cur = np.full((c, 64), far, np.int64)
    diag = np.where(lane == 0, 0, far).astype(np.int64)
    g = np.zeros(64, np.int64)
    skip = 3 - (end - 1) % 4
    last = np.full(64, skip + la, np.int64)
    vend = skip + end + la
    at = ((end - 1) >> 2) - lane
    load = lambda: np.where(at >= 0, words[np.clip(at, 0, len(words) - 1)], 0)   # noqa: E731
    w = load()
    steps = 0
    for v0 in range(0, vend, 256):
        lv = (((w & 0xFF) << 24) | ((w & 0xFF00) << 8) | ((w >> 8) & 0xFF00) | ((w >> 24) & 0xFF)) ^ 0x80808080
        at = at - 64
        w = load()
        block = min(vend - v0, 256)
        m0 = m1 = np.zeros(64, np.int64)
        for s in range(skip if v0 == 0 else 0, block):
            up = np.concatenate(([far], cur[c - 1][:-1]))
            g = np.concatenate(([(int(lv[s >> 2]) >> (8 * (s & 3))) & 0xFF], g[:-1]))
            d, u = diag, up
            for i in range(c):
                left = cur[i].copy()
                u = _msad(g, k[i], np.minimum(np.minimum(d, u), left))
                d, cur[i] = left, u
            diag = up
            last = np.where(cur[track] == cost, v0 + s, last)
            steps += 1
            if s >= min(block, 252):
                m0, m1 = m1, cur.min(axis=0)
        if block == 256 and not (np.minimum(m0, m1) <= cost).any():
            break
        assert int(cur.max()) < 1 << 31, "a register wrapped"
        cur = np.minimum(cur, far)
        diag = np.minimum(diag, far)
    return end - 1 - (int(last[la]) - skip - la), steps


# ---- the catalogue ------------------------------------------------------------------------------------------------------------------------
RUNS = (1, 3, 255, 256, 257, 600)        # a run of the query's first level in front of a plant: around the loader's block of 256 steps
LONG_RUN, LONG_START = 50_000, LR.LONG_END + 2 - 3 * 700 - 50_000


class Call(LR.Call):
    """locate_ref.Call; planted: {(read, target): (cost, end, start)}"""


def _planted(n, seed):
    """one distinct-level query of n levels and its plants; stride 2 048"""
    p = Call("span-planted-%d" % n, 640, 32.0, 2048, seed)
    L = 2048
    q = LR.distinct_levels(p.rng, n)
    ri = p.read(q)
    bg = p.rng.integers(90, 128, L)
    # its very start, its very end, and so that the walk back crosses a seam of the loader's blocks (256 levels back from the end)
    for at in (0, L - n, 1000 - n // 2):
        p.planted[(ri, p.target(LR.plant(bg, at, q)))] = (0, at + n, at)
    p.planted[(ri, p.target(LR.plant(bg, 30, np.repeat(q, 3))))] = (0, 30 + 3 * n - 2, 30)       # every level tripled
    p.planted[(ri, p.target(LR.plant(LR.plant(bg, 10, q), 1100, q)))] = (0, 10 + n, 10)            # two equal plants: the first
    for r in RUNS:   # a run of the FIRST level directly in front: the path sits on it, the start moves to the run's first level
        at = 700
        p.planted[(ri, p.target(LR.plant(LR.plant(bg, at, q), at - r, np.full(r, q[0]))))] = (0, at + n, at - r)
        p.planted[(ri, p.target(LR.plant(LR.plant(bg, r, q), 0, np.full(r, q[0]))))] = (0, r + n, 0)   # ... reaching level 0: out of target
    # a run that does not touch the plant (one level of background between them): the start does not move
    p.planted[(ri, p.target(LR.plant(LR.plant(bg, 700, q), 699 - 40, np.full(40, q[0]))))] = (0, 700 + n, 700)
    return p


def _edges():
    p = Call("span-edges", 640, 32.0, 2048, 4231)
    L = 2048
    # end - 1 at every residue mod 4, on both sides of a boundary of 256 levels
    q = LR.distinct_levels(p.rng, 17)
    ri = p.read(q)
    bg = p.rng.integers(90, 128, L)
    for e1 in (253, 254, 255, 256, 257, 258, 259, 511, 512):
        p.planted[(ri, p.target(LR.plant(bg, e1 - 16, q)))] = (0, e1 + 1, e1 - 16)
    # a constant query against an equal constant target
    p.planted[(p.read(np.full(64, 5)), p.target(np.full(300, 5)))] = (0, 1, 0)
    # valid 0 and above N; refused target_len beside the good rows
    p.read(LR.signal_levels(p.rng, 40), valid=0)
    p.read(LR.signal_levels(p.rng, 640), valid=5000)
    p.read(LR.signal_levels(p.rng, 640), valid=0xFFFFFFFF)
    p.target(LR.signal_levels(p.rng, 40), length=0)
    p.target(LR.signal_levels(p.rng, 40), length=2049)
    p.target(LR.signal_levels(p.rng, 40), length=0xFFFFFFFF)
    return p


def _extremes():
    e = Call("span-extremes", 64, 1.0, 304, 4232)
    lo, hi = e.target(np.full(300, -128)), e.target(np.full(304, 127))
    q_hi, q_lo = e.read(np.full(64, 127)), e.read(np.full(9, -127))
    e.planted[(q_hi, lo)] = (255 * 64, 1, 0)
    e.planted[(q_lo, lo)] = (1 * 9, 1, 0)
    e.planted[(q_lo, hi)] = (254 * 9, 1, 0)
    e.planted[(q_hi, hi)] = (0, 1, 0)
    return e


def _long():
    """a walk back of more than 50 000 steps across the 65 536 line: the tripled plant of locate_ref's long call with 50 000 levels of the
    query's first level in front of it"""
    g = Call("span-long", 704, 32.0, 70_016, 4233)
    q = LR.distinct_levels(g.rng, 700)
    ri = g.read(q)
    bg = g.rng.integers(90, 128, LR.LONG_L)
    at = LR.LONG_END + 2 - 3 * 700
    t = LR.plant(LR.plant(bg, at, np.repeat(q, 3)), at - LONG_RUN, np.full(LONG_RUN, q[0]))
    g.planted[(ri, g.target(t))] = (0, LR.LONG_END, LONG_START)
    return g


@functools.lru_cache(maxsize=None)
def catalogue():
    """locate_ref's whole catalogue (its planted answers carry no start) and behind it the calls of this rule"""
    return list(LR.catalogue()) + [_planted(17, 4235), _planted(129, 4236), _planted(600, 4237), _edges(), _extremes(), _long()]


@functools.lru_cache(maxsize=None)
def expected(index):
    """the spans of catalogue()[index], computed once"""
    c = catalogue()[index]
    query, valid, target, target_len = c.arrays()
    out = spans(query, valid, c.quant, target, target_len)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def sweep_expected():
    """the spans of locate_ref's dense sweep"""
    query, valid, target, target_len, _ = LR.sweep()
    out = spans(query, valid, 32.0, target, target_len)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tie_sweep(top=136, stride=144):
    """a second dense sweep, every n = 1 ... top against every L = 1 ... top, over levels of +-2, where many paths tie -> (query, valid,
    target, target_len, spans)"""
    rng = np.random.default_rng(4234)
    query = np.full((top, top), np.nan, np.float32)
    target = rng.integers(-128, 128, (top, stride)).astype(np.int8)
    for i in range(top):
        n = i + 1
        query[i, :n] = rng.integers(-2, 3, n).astype(np.float32) / np.float32(32.0)
        target[i, :n] = np.repeat(rng.integers(-2, 3, n // 3 + 1), 3)[:n] if i % 2 else rng.integers(-2, 3, n)
    lens = np.arange(1, top + 1, dtype=np.uint32)
    want = spans(query, lens, 32.0, target, lens)
    for a in (query, target, want):
        a.setflags(write=False)
    return query, lens, target, lens, want
