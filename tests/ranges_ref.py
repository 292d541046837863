"""Reference for per-read sample ranges (include/vbz_gpu.h: vbz_gpu_sample_ranges), pure numpy: the range is clamped, the signal sliced,
and the slice is one read to the existing statements -- the chunking rules of pod5_reads_ref and the statistics of norm_ref.  A POD5 read
of several rows is its concatenated rows."""
import numpy as np

import norm_ref as R
import pod5_reads_ref as PR

STATS_RANGE, STATS_READ = 0, 1
TO_END = 0xFFFFFFFF


def clamp(T, begin=None, end=None):
    """(b, e) of a read of T samples: e = min(end, T), b = min(begin, e); None is the NULL table (0 / T)"""
    e = min(T if end is None else int(end), T)
    b = min(0 if begin is None else int(begin), e)
    return b, e


def range_samples(samples, begin=None, end=None):
    """vbz_gpu_range_samples_batch: T' per read; a count of 2^31 or more (an error code) passes through.  begin / end: per-read sequences or None"""
    out = []
    for i, T in enumerate(samples):
        T = int(T)
        if T >= 1 << 31:
            out.append(T)
            continue
        b, e = clamp(T, None if begin is None else begin[i], None if end is None else end[i])
        out.append(e - b)
    return out


def sliced(x, begin=None, end=None):
    b, e = clamp(len(x), begin, end)
    return np.asarray(x)[b:e]


def chunk_rows(x, begin, end, L, S, mode, end_align, o, s, pad, dtype):
    """(starts relative to b, the [K(T'), L] chunk rows' bits) of the range of the signal x (int16, or uint16 for unsigned samples)"""
    return PR.chunk_rows(sliced(x, begin, end), L, S, mode, end_align, o, s, pad, dtype)


def stats_values(x, begin, end, stats):
    """the values the statistics are taken over"""
    return np.asarray(x) if stats == STATS_READ else sliced(x, begin, end)


def shift_scale(x, begin, end, norm, stats=STATS_RANGE):
    """(shift, scale, the store's offset, the store's scale'), float32 each; x int16 or uint16 as the samples are"""
    v = stats_values(x, begin, end, stats)
    return R.constants(*R.stats(v, norm), norm)


def norm_chunk_rows(x, begin, end, L, S, mode, end_align, norm, stats, pad, dtype):
    """the normalised chunk rows of the range: (starts, rows, shift, scale)"""
    shift, scale, o, s = shift_scale(x, begin, end, norm, stats)
    starts, rows = chunk_rows(x, begin, end, L, S, mode, end_align, o, s, pad, dtype)
    return starts, rows, shift, scale


def pod5_signals(rows, first_row):
    """POD5 reads of several rows: every read's concatenated signal, to be passed to the functions above with the read's range"""
    return PR.read_signals(rows, first_row)
