"""numpy statement of the signal trim of include/vbz_gpu.h (vbz_gpu_trim), on top of norm_ref and ranges_ref: the threshold from the
read's {shift, scale} in float64 with every operation rounded once (Python floats: no fused multiply-add), the windows' counts of high
samples, and the walk over them.  A POD5 read of several rows is its concatenated rows.  Also the generator of the reads the GPU tests
use: a noisy baseline with a plateau in front, in the middle, nowhere, or one that never comes down."""
import numpy as np

import norm_ref as R
import pod5_reads_ref as PR
import ranges_ref as G

REJECT_AT_END = 1
MAX_WINDOWS = 4096

# (window, min_elements, min_trim, max_samples, threshold_factor, max_fraction, flags)
DEFAULT = (40, 3, 10, 8000, 2.4, 1.0, 0)


def threshold(shift, scale, f):
    """thr = float64(shift) + float64(f) * float64(scale) for the float32 shift, scale and f: one multiply, then one add"""
    return R.f64(shift) + R.f64(f) * R.f64(scale)


def trim(x, thr, W, m, t0, M, max_fraction=1.0, flags=0, T=None):
    """the trim point of the read's values x (int16 or uint16) under the threshold thr.  T: the read's sample count where x holds only
    its first samples (min(M, T) of them or more: the rule looks at no other)"""
    x = np.asarray(x)
    T = len(x) if T is None else int(T)
    N = min(int(M), T)
    nW = (N - t0) // W if N > t0 else 0
    none = min(t0, T)
    if nW == 0:
        return none
    high = (x[t0 : t0 + nW * W].astype(np.float64) > thr).reshape(nW, W)
    opens = np.flatnonzero(high.sum(axis=1) > m)           # windows with MORE than m high samples
    if opens.size == 0:
        return none                                        # no peak
    stops = np.flatnonzero(~high[opens[0] :, -1])          # at or behind the opening window: the last sample is not high
    if stops.size == 0:
        return none                                        # the peak never comes down
    e = t0 + (int(opens[0]) + int(stops[0]) + 1) * W
    if (flags & REJECT_AT_END) and e >= N:
        return none
    if float(e) > R.f64(max_fraction) * float(T):
        return none
    return e


def begin(x, norm, trim_params=DEFAULT, stat_begin=None, stat_end=None, stats=G.STATS_RANGE):
    """begin[i] of the read x (int16, or uint16 for unsigned samples): the statistics over the range [stat_begin, stat_end) (or, with
    stats = STATS_READ, the whole read) give the threshold; the trim looks at the whole read"""
    W, m, t0, M, f, max_fraction, flags = trim_params
    shift, scale, _, _ = G.shift_scale(x, stat_begin, stat_end, norm, stats)
    return trim(x, threshold(shift, scale, f), W, m, t0, M, max_fraction, flags)


def pod5_begins(rows, first_row, norm, trim_params=DEFAULT, stat_begin=None, stat_end=None, stats=G.STATS_RANGE, signed=True):
    """the begin table of POD5 reads of several rows: per READ, over its concatenated signal; stat_begin / stat_end per read or None"""
    out = []
    for k, x in enumerate(PR.read_signals(rows, first_row)):
        v = x if signed else x.view(np.uint16)
        out.append(begin(v, norm, trim_params, None if stat_begin is None else stat_begin[k], None if stat_end is None else stat_end[k], stats))
    return out


def windows_ok(trim_params):
    """whether a read's windows fit the device's counting slab (the host refuses the others)"""
    W, _, t0, M = trim_params[:4]
    return (M - min(t0, M)) // W <= MAX_WINDOWS


# ---- the reads of the GPU tests ------------------------------------------------------------------------------------------------------
GPU_SIZES = [0, 1, 9, 10, 11, 49, 50, 51, 511, 513, 2047, 2048, 2049, 4101, 7999, 8000, 8001, 8010, 8050, 20_000]
GPU_SEED = 7
KINDS = ("front", "middle", "none", "front", "middle", "stuck")   # the reads generated per size, in this order


def make_read(rng, T, kind, level=400):
    """int16 bits of a read of T samples: baseline level + 12 N(0, 1), rounded, with a +150 plateau: "front" from sample 0, "middle"
    inside the first min(T, 8000) samples, "none", or "stuck" (from a point of the prefix to the read's end).  level = 400 is an int16
    signal; a level beyond 32 767 is a uint16 signal whose bits are returned as int16"""
    x = np.rint(level + 12.0 * rng.standard_normal(T))
    P = min(T, 8000)
    if kind == "front":
        x[: int(rng.integers(P // 8, P // 3 + 1))] += 150
    elif kind == "middle":
        a = int(rng.integers(P // 4, P // 2 + 1))
        x[a : a + int(rng.integers(P // 16, P // 4 + 1))] += 150
    elif kind == "stuck":
        x[int(rng.integers(0, P // 2 + 1)) :] += 150
    return x.astype(np.int64).astype(np.uint16).view(np.int16)


def gpu_reads(seed=GPU_SEED, sizes=GPU_SIZES, level=400):
    """the reads of the GPU tests' size grid: len(KINDS) reads per size"""
    rng = np.random.default_rng(seed)
    return [make_read(rng, T, kind, level) for T in sizes for kind in KINDS]
