"""The raw trim call for the signal-trim tests on the MI355X (test_gpu_trim, test_gpu_foreign_streams): one call with its begin table
between guard words, and its check against trim_ref, with ranges_ref's constants kept per (read, norm, range).  A plain module: every
assert carries its operands."""
import ctypes

import numpy as np
import torch

import ranges_ref as G
import trim_ref as T
from typed_support import NORMS, full, ranges_struct, trim_struct, u32
from vbz_compression_amd import _lib

GUARD = 5
GUARD_WORD = 0x5A5A5A5A


def guarded(c, n):
    """a table of n words between GUARD guard words on either side: (the whole tensor, the pointer of entry 0)"""
    t = torch.full((n + 2 * GUARD,), GUARD_WORD, dtype=torch.int32, device=c.device)
    return t, t.data_ptr() + 4 * GUARD


def table_and_guards(t, n):
    host = u32(t)
    assert (host[:GUARD] == GUARD_WORD).all() and (host[GUARD + n :] == GUARD_WORD).all(), "a guard word of the begin table was written"
    return host[GUARD : GUARD + n].tolist()


_consts = {}


def constants(x, norm, b, e, stats):
    """ranges_ref.shift_scale, kept per (read, norm, range): the sort is the reference's cost"""
    key = (x.dtype.str, x.tobytes(), norm, b, e, stats)
    if key not in _consts:
        _consts[key] = G.shift_scale(x, b, e, norm, stats)[:2]
    return _consts[key]


def want_begin(x, norm, p, b=None, e=None, stats=0):
    shift, scale = constants(x, norm, b, e, stats)
    W, m, t0, M, f, mf, flags = p
    return T.trim(x, T.threshold(shift, scale, f), W, m, t0, M, mf, flags), shift, scale


class TrimRun:
    """one raw vbz_gpu_signal_trim_batch call and its check against trim_ref"""

    def __init__(self, fr, p=T.DEFAULT, norm="med_mad", signed=True, sb=None, se=None, stats=0, with_ss=True, src=None, size=None):
        c = fr.c
        self.fr, self.p, self.norm, self.signed, self.stats = fr, p, NORMS[norm] if isinstance(norm, str) else norm, signed, stats
        n, dev = fr.n, c.device
        self.sb, self.se = full(sb, n), full(se, n)
        self.begin, ptr = guarded(c, n)
        self.result = torch.full((max(n, 1),), -8, dtype=torch.int32, device=dev)
        self.ss = torch.full((max(n, 1), 2), -777.0, dtype=torch.float32, device=dev) if with_ss else None
        b = c._batch(fr.src if src is None else src, fr.off, fr.size if size is None else size, torch.empty(0, dtype=torch.uint8, device=dev), fr.doff,
                     fr.dcap, self.result)
        b.dst, b.dst_bytes = None, fr.dst_bytes
        m = self.norm[1].c_struct()
        t = trim_struct(p)
        g, keep = ranges_struct(c, sb, se, stats)
        ranged = sb is not None or se is not None
        torch.cuda.synchronize()
        self.rc = c.L.vbz_gpu_signal_trim_batch(c.ctx, ctypes.byref(b), ctypes.byref(fr.opts), int(fr.sized), int(signed), ctypes.byref(m),
                                                ctypes.byref(g) if ranged else None, ctypes.byref(t), self.ss.data_ptr() if with_ss else None, ptr)
        c.synchronize()
        self.err = c.L.vbz_gpu_last_error(c.ctx)

    def check(self, expect=None):
        """result[] (expect[i]: an error verdict), begin[] and shift_scale of every read, the guard words"""
        assert self.rc == 0, self.err
        fr = self.fr
        res = u32(self.result)
        got = table_and_guards(self.begin, fr.n)
        ss = self.ss.cpu().numpy() if self.ss is not None else None
        for i in range(fr.n):
            want_res = 2 * fr.T[i] if not (expect and i in expect) else expect[i]
            assert int(res[i]) == want_res, (i, hex(int(res[i])), hex(want_res))
            if _lib.is_error(want_res):
                assert got[i] == 0, ("begin of a failed read", i, got[i])
                continue
            x = fr.reads[i] if self.signed else fr.reads[i].view(np.uint16)
            want, shift, scale = want_begin(x, self.norm[0], self.p, self.sb[i], self.se[i], self.stats)
            assert got[i] == want, ("begin", i, "T", fr.T[i], self.p, self.norm[1].method, self.signed, self.sb[i], self.se[i], self.stats, got[i], want)
            if ss is not None:
                assert (ss[i][0].view(np.uint32), ss[i][1].view(np.uint32)) == (shift.view(np.uint32), scale.view(np.uint32)), ("shift_scale", i, ss[i], shift, scale)
        return got
