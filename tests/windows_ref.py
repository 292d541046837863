"""Reference for caller-listed signal windows (include/vbz_gpu.h: vbz_gpu_windows), pure numpy: the range is clamped and the signal sliced
as ranges_ref does, the slice is converted by signal_ref's typed store, and position p of the row of a window starting at s holds converted
sample s + p of the slice when 0 <= s + p < T', the pad bits otherwise.  A POD5 read of several rows is its concatenated rows."""
import numpy as np

import ranges_ref as G
import signal_ref as SR


def window_rows(x, begin, end, starts, L, o, s, pad, dtype):
    """the [len(starts), L] rows' bits of the windows `starts` (any integers) of the range of the signal x (int16, or uint16 for unsigned
    samples) calibrated with (o, s)"""
    bits = SR.typed_bits(G.sliced(x, begin, end), o, s, dtype)
    T = len(bits)
    idx = np.asarray(starts, np.int64).reshape(-1, 1) + np.arange(L, dtype=np.int64)[None, :]
    out = np.full(idx.shape, SR.pad_bits(pad, dtype), bits.dtype)
    m = (idx >= 0) & (idx < T)
    out[m] = bits[idx[m]]
    return out


def norm_window_rows(x, begin, end, starts, L, norm, stats, pad, dtype):
    """the normalised rows of the range's windows: (rows, shift, scale)"""
    shift, scale, o, s = G.shift_scale(x, begin, end, norm, stats)
    return window_rows(x, begin, end, starts, L, o, s, pad, dtype), shift, scale
