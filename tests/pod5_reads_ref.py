"""Reference for POD5 reads of several rows (include/vbz_gpu.h: vbz_gpu_pod5_reads), pure numpy on top of pod5_ref and norm_ref: a read
is the concatenation of its rows; its chunks are vbz_gpu_chunking's for the concatenated signal and its statistics norm_ref's."""
import numpy as np

import norm_ref as R
from signal_ref import chunk_rows, chunk_starts, pad_bits, typed_bits   # noqa: F401  (the one statement of each; a read's rows concatenated are a signal to them)


def bounds(first_row, n_rows):
    """first_row (the first row of every read) -> the n_reads + 1 table the C struct takes"""
    return [int(v) for v in first_row] + [int(n_rows)]


def read_signals(rows, first_row):
    """the concatenated int16 signal of every read"""
    b = bounds(first_row, len(rows))
    return [np.concatenate([np.asarray(x, np.int16) for x in rows[b[k] : b[k + 1]]] + [np.zeros(0, np.int16)]) for k in range(len(first_row))]


def shift_scale(x, norm, signed=True):
    """(shift, scale) float32 of the read, and the store's constants (offset, scale') as norm_ref gives them"""
    v = np.asarray(x, np.int16) if signed else np.asarray(x, np.int16).view(np.uint16)
    shift, scale = R.shift_scale(v, norm)
    _, _, so, sc = R.constants(*R.stats(v, norm), norm)
    return shift, scale, so, sc
