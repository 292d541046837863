"""Reference for signal events (include/vbz_gpu.h: vbz_gpu_events), pure numpy: the range is clamped and the signal sliced as ranges_ref
does; event c of a read's sorted starts covers the positions [min(start[c], T'), min(start[c + 1], T')) of the slice, the last one up to
T'.  The moments are exact integers from np.int64 / np.uint64 cumulative sums; the record is formed from them in np.float64, one rounding
per operation (numpy's ufuncs fuse nothing), and rounded once to float32.  A POD5 read of several rows is its concatenated rows."""
import numpy as np

import ranges_ref as G


def bounds(T, starts):
    """(a, z) per event, uint64: the clamped positions each event covers in a signal of T samples (starts: sorted, 0 ... 0xFFFFFFFF)"""
    st = np.minimum(np.asarray(starts, np.uint64).reshape(-1), np.uint64(T))
    return st, np.concatenate([st[1:], np.asarray([T], np.uint64)]) if len(st) else st


def moments(x, starts):
    """(n uint32, S1 int64, S2 uint64) per event of the signal x (int16, or uint16 for unsigned samples)"""
    x = np.asarray(x)
    a, z = bounds(len(x), starts)
    v = x.astype(np.int64)
    c1 = np.concatenate([np.zeros(1, np.int64), np.cumsum(v, dtype=np.int64)])
    c2 = np.concatenate([np.zeros(1, np.uint64), np.cumsum((v * v).astype(np.uint64), dtype=np.uint64)])
    a, z = a.astype(np.int64), z.astype(np.int64)
    return (z - a).astype(np.uint32), c1[z] - c1[a], c2[z] - c2[a]


def records(n, S1, S2, o, s):
    """(mean float32, sd float32) of the events' moments under the read's constants (o, s): float64, every operation rounded once"""
    o, s = np.float64(np.float32(o)), np.float64(np.float32(s))
    live = n > 0
    nd = np.where(live, n, 1).astype(np.float64)
    m = S1.astype(np.float64) / nd
    q = S2.astype(np.float64) / nd
    mm = m * m
    v = q - mm
    v = np.where(v < 0.0, 0.0, v)
    r = np.sqrt(v)
    with np.errstate(over="ignore"):   # (a tiny normalisation scale: the float32 record is inf, on the device too)
        mean = ((m + o) * s).astype(np.float32)
        sd = (r * np.abs(s)).astype(np.float32)
    zero = np.float32(0.0)
    return np.where(live, mean, zero), np.where(live, sd, zero)


def event_rows(x, begin, end, starts, o, s):
    """(the [len(starts), 4] uint32 rows {mean bits, sd bits, n, 0}, the [len(starts), 2] int64 moments {S1, S2's bits}) of the events
    `starts` of the range of the signal x calibrated with (o, s)"""
    n, S1, S2 = moments(G.sliced(x, begin, end), starts)
    mean, sd = records(n, S1, S2, o, s)
    rows = np.zeros((len(n), 4), np.uint32)
    rows[:, 0], rows[:, 1], rows[:, 2] = mean.view(np.uint32), sd.view(np.uint32), n
    return rows, np.stack([S1, S2.view(np.int64)], axis=1) if len(n) else np.zeros((0, 2), np.int64)


def norm_event_rows(x, begin, end, starts, norm, stats):
    """the rows under the read's own statistics: (rows, moments, shift, scale)"""
    shift, scale, o, s = G.shift_scale(x, begin, end, norm, stats)
    rows, mom = event_rows(x, begin, end, starts, o, s)
    return rows, mom, shift, scale
