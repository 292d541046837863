"""The one numpy statement of the typed store and of the chunk rule (include/vbz_gpu.h: vbz_gpu_signal_format, vbz_gpu_chunking): what a
16-bit sample becomes, ((float32)x + offset) * scale rounded once to the output type, and where the chunks of a read begin.  Every other
reference (pod5_reads_ref, ranges_ref) and every device test is built on these; tests/test_signal_ref.py holds the conversion to an
independent formulation.  Output types are the strings "f32", "f16", "bf16"."""
import numpy as np


def typed_bits(x, o, s, dtype):
    """bits of ((float32)x + o) * s rounded once to dtype: uint32 or uint16.  x: the samples as the values they are (int16, or uint16 for
    unsigned samples); o, s: float32 scalars or per-sample arrays"""
    y = (np.asarray(x).astype(np.float32) + np.float32(o)) * np.float32(s)
    if dtype == "f32":
        return y.view(np.uint32)
    if dtype == "f16":
        return y.astype(np.float16).view(np.uint16)
    u = y.view(np.uint32).astype(np.uint64)   # bfloat16: round to nearest even on the upper half; a NaN keeps its upper half, made quiet
    return np.where(np.isnan(y), (u >> 16) | 0x40, (u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def is_nan_bits(bits, dtype):
    if dtype == "f32":
        return np.isnan(bits.view(np.float32))
    if dtype == "f16":
        return np.isnan(bits.view(np.float16))
    return ((bits & 0x7F80) == 0x7F80) & ((bits & 0x7F) != 0)


def pad_bits(pad, dtype):
    return typed_bits(np.zeros(1, np.int16), pad, 1.0, dtype)[0]


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
    assert all(a < b for a, b in zip(starts, starts[1:])), (T, L, S, mode, end_align, starts[-2:])
    return starts


def table_of(Ts, L, S, mode, end_align):
    """chunk_first of reads of Ts samples: n + 1 entries, int64"""
    counts = [len(chunk_starts(int(t), L, S, mode, end_align)) for t in Ts]
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def ref_rows(bits, T, L, S, mode, end_align, padb):
    """the [K, L] chunk rows of one read's converted samples `bits` (T of them), pad bits behind the read's end"""
    starts = np.asarray(chunk_starts(T, L, S, mode, end_align), np.int64)
    idx = starts[:, None] + np.arange(L, dtype=np.int64)[None, :]
    out = np.full(idx.shape, padb, bits.dtype)
    m = idx < T
    out[m] = bits[idx[m]]
    return out


def chunk_rows(x, L, S, mode, end_align, o, s, pad, dtype):
    """(starts, the [K, L] chunk rows' bits) of the signal x calibrated with (o, s)"""
    bits = typed_bits(x, o, s, dtype)
    return chunk_starts(len(x), L, S, mode, end_align), ref_rows(bits, len(x), L, S, mode, end_align, pad_bits(pad, dtype))
