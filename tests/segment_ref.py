"""Reference for signal segmentation (include/vbz_gpu.h: vbz_gpu_segmentation), pure numpy: the two-window t-statistic in exact integers
(int64 cumulative sums), float64 scores, and the local non-maximum suppression.  The signal is the slice ranges_ref.sliced gives; a POD5
read of several rows is its concatenated rows.  Parameters travel as the tuple P = (w1, w2, t1, t2, r)."""
import numpy as np

import ranges_ref as G

DEFAULT = (3, 6, 4.0, 9.0, 2)


def detector(x, w, t):
    """s_d[0 ... T]: (float64(N) / float64(D)) / (float64(t) float64(t)) for w <= q <= T - w, else 0"""
    x = np.asarray(x).astype(np.int64)
    T = len(x)
    s = np.zeros(T + 1, np.float64)
    if w == 0 or T < 2 * w:
        return s
    c1 = np.concatenate([[0], np.cumsum(x)])
    c2 = np.concatenate([[0], np.cumsum(x * x)])
    q = np.arange(w, T - w + 1)
    A, B = c1[q] - c1[q - w], c1[q + w] - c1[q]
    A2, B2 = c2[q] - c2[q - w], c2[q + w] - c2[q]
    N = w * (A - B) ** 2
    D = np.maximum(w * (A2 + B2) - A * A - B * B, 1)
    tt = np.float64(np.float32(t)) * np.float64(np.float32(t))
    s[q] = (N.astype(np.float64) / D.astype(np.float64)) / tt
    return s


def scores(x, P):
    """s[0 ... T] = max(s_1, s_2)"""
    w1, w2, t1, t2, r = P
    return np.maximum(detector(x, w1, t1), detector(x, w2, t2))


def boundaries(s, r):
    """the boundaries among positions 1 ... T - 1 of the scores s[0 ... T]: s[q] >= 1, larger than the r scores in front of it, no smaller
    than the r scores behind it (up to s[T])"""
    T = len(s) - 1
    if T < 2:
        return np.zeros(0, np.int64)
    pad = np.full(r, -1.0)
    p = np.concatenate([pad, s, pad])   # p[q + r] = s[q]
    win = np.lib.stride_tricks.sliding_window_view(p, 2 * r + 1)   # win[q] = s[q - r ... q + r]
    left, right = win[:, :r].max(axis=1), win[:, r + 1 :].max(axis=1)
    ok = (s >= 1.0) & (s > left) & (s >= right)
    ok[0] = ok[T] = False
    return np.flatnonzero(ok)


def starts(x, begin=None, end=None, P=DEFAULT):
    """the rows of the read: [] for an empty signal, else 0 and the boundaries (uint32)"""
    v = G.sliced(x, begin, end)
    if len(v) == 0:
        return np.zeros(0, np.uint32)
    return np.concatenate([[0], boundaries(scores(v, P), P[4])]).astype(np.uint32)


def tables(reads, begin=None, end=None, P=DEFAULT):
    """(event_first int64 [n + 1], the reads' starts) as the call writes them"""
    st = [starts(x, None if begin is None else begin[i], None if end is None else end[i], P) for i, x in enumerate(reads)]
    return np.concatenate([[0], np.cumsum([len(v) for v in st])]).astype(np.int64), st


def max_rows(T, r):
    return 2 + T // (r + 1)
