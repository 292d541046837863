"""The raw window calls for the signal-window tests on the MI355X (test_gpu_windows, test_gpu_windows_refusals): one call into a canary
arena with guard rows behind it, and its check against windows_ref -- over reads (typed_support.Frames) and over POD5 reads of several
rows (typed_support.Call).  A plain module: every assert carries its operands."""
import ctypes

import numpy as np
import torch

import pod5_reads_ref as PR
import ranges_ref as G
import windows_ref as W
from typed_support import CANARY, ELEM, PAD, Call, device_tables, fmt, full, ranges_struct, u32
from vbz_compression_amd import _lib


def windows_struct(c, first, flat, L, rows=None, pad=PAD, flags=0, reserved=0):
    """(vbz_gpu_windows, its tables): first = window_first (n + 1 entries), flat = start[] (any integers that fit int32)"""
    first_d = torch.from_numpy(np.asarray(first, np.int64)).to(c.device)
    flat_d = torch.from_numpy(np.asarray(flat, np.int64).astype(np.int32)).to(c.device)
    w = _lib.GpuWindows()
    w.window_len, w.pad, w.window_rows = L, pad, len(flat) if rows is None else rows
    w.window_first, w.start, w.flags, w.reserved = first_d.data_ptr(), flat_d.data_ptr() if len(flat) else None, flags, reserved
    return w, [first_d, flat_d]


def table_and_flat(starts):
    """per-read lists of starts -> (window_first, start[])"""
    first = np.concatenate([[0], np.cumsum([len(s) for s in starts])]).astype(np.int64)
    return first, [int(v) for s in starts for v in s]


class WinRun:
    """one raw vbz_gpu_decompress_windows_batch call and its check.  starts[i]: read i's sorted window starts.  first / flat / rows: other
    tables than those of `starts` (a read whose entries differ is then expected to fail).  guard: canary rows behind the arena's last row"""

    def __init__(self, fr, starts, L, dtype="f16", begin=None, end=None, norm=None, stats=0, signed=True, offset=None, scale=None, first=None,
                 flat=None, rows=None, src=None, guard=3):
        c = fr.c
        self.fr, self.starts, self.L, self.dtype, self.norm, self.stats, self.signed, self.guard = fr, starts, L, dtype, norm, stats, signed, guard
        n, dev = fr.n, c.device
        self.bg, self.en = full(begin, n), full(end, n)
        t, fl = table_and_flat(starts)
        self.table = t if first is None else np.asarray(first, np.int64)
        self.flat = fl if flat is None else flat
        self.rows = len(self.flat)
        self.out = torch.full(((self.rows + guard) * L * ELEM[dtype],), CANARY, dtype=torch.uint8, device=dev)
        self.result = torch.full((max(n, 1),), -8, dtype=torch.int32, device=dev)
        self.ss = torch.full((max(n, 1), 2), -777.0, dtype=torch.float32, device=dev)
        self.o = np.zeros(n, np.float32) if offset is None else np.asarray(offset, np.float32)
        self.s = np.ones(n, np.float32) if scale is None else np.asarray(scale, np.float32)
        f = fmt(dtype, signed)
        self.keep = device_tables(c, f, offset, scale)
        b = c._batch(fr.src if src is None else src, fr.off, fr.size, torch.empty(0, dtype=torch.uint8, device=dev), fr.doff, fr.dcap, self.result)
        b.dst, b.dst_bytes = None, fr.dst_bytes
        w, keep = windows_struct(c, self.table, self.flat, L, rows)
        self.keep += keep
        m = norm[1].c_struct() if norm is not None else None
        g, keep = ranges_struct(c, begin, end, stats)
        self.keep += keep
        torch.cuda.synchronize()
        self.rc = c.L.vbz_gpu_decompress_windows_batch(c.ctx, ctypes.byref(b), ctypes.byref(fr.opts), int(fr.sized), ctypes.byref(f), ctypes.byref(w),
                                                       self.out.data_ptr(), ctypes.byref(m) if m is not None else None,
                                                       self.ss.data_ptr() if m is not None else None,
                                                       ctypes.byref(g) if (begin is not None or end is not None) else None)
        c.synchronize()
        self.err = c.L.vbz_gpu_last_error(c.ctx)

    def bits(self):
        return self.out.cpu().numpy().view(np.uint32 if self.dtype == "f32" else np.uint16).reshape(self.rows + self.guard, self.L)

    def values(self, i):
        x = self.fr.reads[i]
        return x if self.signed else x.view(np.uint16)

    def check(self, expect=None, skip=()):
        """verdicts (expect[i]: another verdict than T x E), every passing read's rows and constants, the canary everywhere else"""
        assert self.rc == 0, self.err
        fr, E = self.fr, ELEM[self.dtype]
        res = u32(self.result)
        got = self.bits()
        ss = self.ss.cpu().numpy()
        owned = np.zeros(self.rows + self.guard, bool)
        for i in range(fr.n):
            want_res = fr.T[i] * E if not (expect and i in expect) else expect[i]
            assert int(res[i]) == want_res, (i, hex(int(res[i])), hex(want_res))
            if i in skip:   # (rows left unspecified: a stream that failed while it was stored)
                owned[self.table[i] : self.table[i + 1]] = True
            if _lib.is_error(want_res) or i in skip:
                continue
            x = self.values(i)
            if self.norm is not None:
                want, shift, scale = W.norm_window_rows(x, self.bg[i], self.en[i], self.starts[i], self.L, self.norm[0], self.stats, PAD, self.dtype)
                assert (ss[i][0].view(np.uint32), ss[i][1].view(np.uint32)) == (shift.view(np.uint32), scale.view(np.uint32)), (
                    "shift_scale", i, fr.T[i], self.bg[i], self.en[i], ss[i], shift, scale)
            else:
                want = W.window_rows(x, self.bg[i], self.en[i], self.starts[i], self.L, self.o[i], self.s[i], PAD, self.dtype)
            lo, hi = int(self.table[i]), int(self.table[i + 1])
            assert hi - lo == len(self.starts[i]), (i, lo, hi, len(self.starts[i]))
            bad = np.argwhere(got[lo:hi] != want)
            assert bad.size == 0, (self.L, self.dtype, "read", i, "T", fr.T[i], "range", self.bg[i], self.en[i], "window, position", bad[:4].tolist(),
                                   "starts", [self.starts[i][k] for k in sorted({int(v[0]) for v in bad[:4]})])
            owned[lo:hi] = True
        assert (got[~owned].view(np.uint8) == CANARY).all(), ("a row outside the passing reads' rows was written", np.argwhere(
            (got[~owned].view(np.uint8) != CANARY).any(axis=1))[:4].tolist())
        return self


class WinCall(Call):
    """one raw vbz_gpu_pod5_decompress_windows_batch call over POD5 reads of several rows; starts[k]: read k's windows"""

    def __init__(self, c, frames, rows, first, starts, L, dtype="f16", begin=None, end=None, norm=None, stats=0, table=None, wfirst=None, flat=None, **kw):
        super().__init__(c, frames, [len(x) for x in rows], PR.bounds(first, len(rows)) if table is None else table, dtype, None, norm=norm, **kw)
        self.sig = G.pod5_signals(rows, first)
        self.starts, self.L, self.norm_p, self.stats = starts, L, norm, stats
        self.bg, self.en = full(begin, len(first)), full(end, len(first))
        t, fl = table_and_flat(starts)
        self.wtable = t if wfirst is None else np.asarray(wfirst, np.int64)
        self.flat = fl if flat is None else flat
        self.wrows = len(self.flat)
        self.out = torch.full(((self.wrows + self.guard) * L * ELEM[dtype],), CANARY, dtype=torch.uint8, device=c.device)
        self.w, self.wkeep = windows_struct(c, self.wtable, self.flat, L)
        self.g, self.gkeep = ranges_struct(c, begin, end, stats)
        self.ranged = begin is not None or end is not None

    def call(self):
        m = ctypes.byref(self.m) if self.m is not None else None
        rc = self.c.L.vbz_gpu_pod5_decompress_windows_batch(self.c.ctx, ctypes.byref(self.b), ctypes.byref(self.opts), ctypes.byref(self.f),
                                                            ctypes.byref(self.reads), ctypes.byref(self.w), self.out.data_ptr(), m,
                                                            self.ss.data_ptr() if self.m is not None else None,
                                                            ctypes.byref(self.g) if self.ranged else None)
        self.c.synchronize()
        return rc

    def bits(self):
        return self.out.cpu().numpy().view(np.uint32 if self.dtype == "f32" else np.uint16).reshape(self.wrows + self.guard, self.L)

    def check(self, norm=None, consts=None, skip=(), refused=()):
        """every read's rows against windows_ref (skip: rows left unspecified; refused: rows that must still hold the canary)"""
        got = self.bits()
        ss = self.ss.cpu().numpy()
        owned = np.zeros(self.wrows + self.guard, bool)
        for k, x in enumerate(self.sig):
            lo, hi = int(self.wtable[k]), int(self.wtable[k + 1])
            if k in skip:
                owned[lo:hi] = True
            if k in skip or k in refused:
                continue
            if norm is not None:
                want, shift, scale = W.norm_window_rows(x, self.bg[k], self.en[k], self.starts[k], self.L, norm, self.stats, PAD, self.dtype)
                assert (ss[k][0].view(np.uint32), ss[k][1].view(np.uint32)) == (shift.view(np.uint32), scale.view(np.uint32)), ("shift_scale", k)
            else:
                want = W.window_rows(x, self.bg[k], self.en[k], self.starts[k], self.L, consts[k][0], consts[k][1], PAD, self.dtype)
            bad = np.argwhere(got[lo:hi] != want)
            assert bad.size == 0, (self.L, self.dtype, "read", k, "T", len(x), "range", self.bg[k], self.en[k], "window, position", bad[:4].tolist())
            owned[lo:hi] = True
        assert (got[~owned].view(np.uint8) == CANARY).all(), "a row outside the passing reads' rows was written"
