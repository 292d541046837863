"""Reference for POD5 reads of several rows (include/vbz_gpu.h: vbz_gpu_pod5_reads), pure numpy on top of pod5_ref and norm_ref: a read
is the concatenation of its rows; its chunks are vbz_gpu_chunking's for the concatenated signal and its statistics norm_ref's."""
import numpy as np

import norm_ref as R


def bounds(first_row, n_rows):
    """first_row (the first row of every read) -> the n_reads + 1 table the C struct takes"""
    return [int(v) for v in first_row] + [int(n_rows)]


def read_signals(rows, first_row):
    """the concatenated int16 signal of every read"""
    b = bounds(first_row, len(rows))
    return [np.concatenate([np.asarray(x, np.int16) for x in rows[b[k] : b[k + 1]]] + [np.zeros(0, np.int16)]) for k in range(len(first_row))]


def chunk_starts(T, L, S, mode, end_align):
    """start samples of the chunks of a read of T samples (mode "pad" or "end")"""
    if T == 0:
        return []
    if T <= L:
        return [0]
    ks = -(-(T - L) // S)
    starts = [k * S for k in range(ks + 1)]
    if mode == "end":
        starts[-1] = min(starts[-1], -(-(T - L) // end_align) * end_align)
    return starts


def typed_bits(x, o, s, dtype):
    """bits of ((float32)x + o) * s rounded once to dtype ("f32", "f16", "bf16"): uint32 or uint16"""
    y = (np.asarray(x).astype(np.float32) + np.float32(o)) * np.float32(s)
    if dtype == "f32":
        return y.view(np.uint32)
    if dtype == "f16":
        return y.astype(np.float16).view(np.uint16)
    u = y.view(np.uint32).astype(np.uint64)   # bfloat16: round to nearest even on the upper half (finite values)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def pad_bits(pad, dtype):
    return typed_bits(np.zeros(1, np.int16), pad, 1.0, dtype)[0]


def chunk_rows(x, L, S, mode, end_align, o, s, pad, dtype):
    """the [K, L] chunk rows (bits) of the signal x calibrated with (o, s)"""
    starts = chunk_starts(len(x), L, S, mode, end_align)
    bits = typed_bits(x, o, s, dtype)
    out = np.full((len(starts), L), pad_bits(pad, dtype), bits.dtype)
    for k, a in enumerate(starts):
        seg = bits[a : a + L]
        out[k, : len(seg)] = seg
    return starts, out


def shift_scale(x, norm, signed=True):
    """(shift, scale) float32 of the read, and the store's constants (offset, scale') as norm_ref gives them"""
    v = np.asarray(x, np.int16) if signed else np.asarray(x, np.int16).view(np.uint16)
    shift, scale = R.shift_scale(v, norm)
    _, _, so, sc = R.constants(*R.stats(v, norm), norm)
    return shift, scale, so, sc
