"""The numpy statement of signal spans (include/vbz_gpu.h: vbz_gpu_spans), written from the header's rule: the threshold in float64 (one
multiply, then one add), the strict comparison on float64 values, the merge of in-positions at most D apart, the length filter behind
the merge, the rows as {begin, end} pairs, the bound -- and the signal builders the tests share: a baseline with planted runs, and noise.
P = (direction, D, m, p0, f); ranges clamp as ranges_ref does."""
import numpy as np

import ranges_ref as G

ABOVE, BELOW = 0, 1
DEFAULT = (ABOVE, 0, 1, 0, 0.0)


def threshold(a, w, f):
    """thr = float64(a) + float64(f) * float64(w) of float32 a, w, f: numpy's float64 multiply and add round to nearest even, unfused"""
    with np.errstate(all="ignore"):
        return np.float64(np.float32(a)) + np.float64(np.float32(f)) * np.float64(np.float32(w))


def is_in(x, thr, direction, p0):
    """one bool per position of the signal x (int16 or uint16 values)"""
    v = np.asarray(x).astype(np.float64)
    with np.errstate(invalid="ignore"):
        hit = v > thr if direction == ABOVE else v < thr
    hit = np.asarray(hit, bool).copy()
    hit[: min(int(p0), len(hit))] = False
    return hit


def merge(hit, D, m):
    """the spans of the in-positions: int64 [k, 2] of {first, last + 1}, ascending"""
    q = np.flatnonzero(hit).astype(np.int64)
    if len(q) == 0:
        return np.zeros((0, 2), np.int64)
    cut = np.flatnonzero(np.diff(q) - 1 > D)              # a new span begins behind q[cut]
    first = np.concatenate([[q[0]], q[cut + 1]])
    last = np.concatenate([q[cut], [q[-1]]])
    keep = last + 1 - first >= m
    return np.stack([first[keep], last[keep] + 1], 1)


def spans(x, begin, end, P, a, w):
    """the spans of read x (its values as the call sees them: int16, or uint16) over its clamped range, level {a, w}"""
    direction, D, m, p0, f = P
    b, e = G.clamp(len(x), begin, end)
    return merge(is_in(np.asarray(x)[b:e], threshold(a, w, f), direction, p0), D, m)


def edges(x, begin, end, P, a, w):
    """the read's words of edge: begin, end, begin, end, ... as uint32"""
    return spans(x, begin, end, P, a, w).reshape(-1).astype(np.uint32)


def tables(reads, P, levels, begin=None, end=None, failed=()):
    """(edge_first int64 [n + 1], the reads' edge words) of a call; levels[i] = (a, w); a read in `failed` owns nothing"""
    n = len(reads)
    bg = [None] * n if begin is None else list(begin)
    en = [None] * n if end is None else list(end)
    ed = [np.zeros(0, np.uint32) if i in failed else edges(x, bg[i], en[i], P, levels[i][0], levels[i][1]) for i, x in enumerate(reads)]
    return np.concatenate([[0], np.cumsum([len(v) for v in ed])]).astype(np.int64), ed


def bound(T, D, m):
    """spans <= (T' + D + 1) / (m + D + 1) by integer division"""
    return (int(T) + D + 1) // (m + D + 1)


def key_bounds(thr, direction, signed):
    """The device's integer form of the comparison, from the header's How: on the 16-bit key u = x + kx (kx = 32 768 for int16, 0 for
    uint16) ABOVE is u >= floor(thr) + 1 + kx and BELOW is u < ceil(thr) + kx, each bound clamped to [0, 65536]; a NaN thr: none.
    -> (lo, hi): in when lo <= u < hi"""
    kx = 32768 if signed else 0
    if np.isnan(thr):
        return 0, 0

    def clamp(h):
        return 65536 if h >= 65536.0 else (int(h) if h > 0.0 else 0)

    if direction == ABOVE:
        return clamp(np.floor(thr) + 1.0 + kx), 65536
    return 0, clamp(np.ceil(thr) + kx)


# ---- signals --------------------------------------------------------------------------------------------------------------------------
def baseline(T, runs, base=400, level=900, dtype=np.int16):
    """a flat baseline with planted runs [(first, last + 1), ...] at `level` (clipped to the signal)"""
    x = np.full(T, base, dtype)
    for a, z in runs:
        x[max(a, 0) : max(min(z, T), 0)] = level
    return x


def noisy(rng, T, runs=(), base=400, sd=30.0, level=1200):
    """Gaussian noise around a baseline, with planted plateaus"""
    x = base + rng.normal(0, sd, T)
    for a, z in runs:
        x[max(a, 0) : max(min(z, T), 0)] = level + rng.normal(0, sd, max(min(z, T), 0) - max(a, 0))
    return np.clip(x, -32768, 32767).astype(np.int16)


def pair(T, s, gap, L, **kw):
    """two runs of L samples whose gap of `gap` positions straddles the seam s (gap 0: one run of 2 L samples across s), as far to the
    right as fits in front of s: the first run ends at or in front of s, the second begins at or behind it"""
    a = max(0, s - gap // 2 - L)
    assert a + L <= s <= a + L + gap and a + 2 * L + gap <= T, (T, s, gap, L)
    return baseline(T, [(a, a + L), (a + L + gap, a + 2 * L + gap)], **kw)


SEAMS = (1000, 1007, 512, 2048)   # a map byte's first and last position, a wavefront's and a tile's first sample


def catalogue(D, m, T=4200):
    """[(name, signal)] for merge gap D and minimum length m >= 2: per seam, pairs of runs of length m and m - 1 with a gap of exactly D
    (they merge) and of D + 1 (they do not) straddling it; single runs that begin or end at both edges of a map byte, of a wavefront
    and of a tile, at position 0 and at T - 1.  A gap wider than the seams' distances (D = 65535) straddles all of them in one read."""
    out = []
    wide = D + 1 + 2 * m > 400
    for s in (SEAMS[-1:] if wide else SEAMS):
        for gap in (D, D + 1):
            for L in (m, m - 1):
                out.append(("pair s%d gap%d L%d" % (s, gap, L), pair(max(T, 2 * L + gap + 11), s, gap, L)))
    for s in (8, 15, 512, 2048):
        out.append(("begins at %d" % s, baseline(T, [(s, s + m + 2)])))
        out.append(("last at %d" % (s - 1 if s % 8 == 0 else s), baseline(T, [((s if s % 8 else s - 1) - m - 1, (s if s % 8 else s - 1) + 1)])))
    out.append(("at 0", baseline(T, [(0, m)])))
    out.append(("at T - 1", baseline(T, [(T - m, T)])))
    out.append(("short at both ends", baseline(T, [(0, m - 1), (T - m + 1, T)])))
    return out
