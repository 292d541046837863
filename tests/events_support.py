"""The raw event calls for the signal-event tests on the MI355X (test_gpu_events, test_gpu_events_refusals): one call into canary arenas
(records and moments) with guard rows behind them, and its check against events_ref -- over reads (typed_support.Frames) and over POD5
reads of several rows (typed_support.Call).  A plain module: every assert carries its operands."""
import ctypes

import numpy as np
import torch

import events_ref as EV
import pod5_reads_ref as PR
import ranges_ref as G
from typed_support import CANARY, Call, device_tables, fmt, full, i32, ranges_struct, u32
from vbz_compression_amd import _lib


def events_struct(c, first, flat, rows=None, flags=0, reserved=0):
    """(vbz_gpu_events, its tables): first = event_first (n + 1 entries), flat = start[] (integers 0 ... 0xFFFFFFFF)"""
    first_d = torch.from_numpy(np.asarray(first, np.int64)).to(c.device)
    flat_d = i32([int(v) for v in flat]).to(c.device)
    ev = _lib.GpuEvents()
    ev.event_rows = len(flat) if rows is None else rows
    ev.event_first, ev.start, ev.flags, ev.reserved = first_d.data_ptr(), flat_d.data_ptr() if len(flat) else None, flags, reserved
    return ev, [first_d, flat_d]


def table_and_flat(starts):
    """per-read lists of starts -> (event_first, start[])"""
    first = np.concatenate([[0], np.cumsum([len(s) for s in starts])]).astype(np.int64)
    return first, [int(v) for s in starts for v in s]


def canaries(c, rows, guard):
    out = torch.full(((rows + guard) * 16,), CANARY, dtype=torch.uint8, device=c.device)
    return out, out.clone()


def compare(got, mom, lo, hi, want, want_mom, what):
    bad = np.argwhere(got[lo:hi] != want)
    assert bad.size == 0, (what, "record row, field", bad[:4].tolist(), got[lo:hi][bad[0][0]].tolist(), want[bad[0][0]].tolist())
    if mom is not None:
        bad = np.argwhere(mom[lo:hi] != want_mom)
        assert bad.size == 0, (what, "moments row, field", bad[:4].tolist(), mom[lo:hi][bad[0][0]].tolist(), want_mom[bad[0][0]].tolist())


class EvRun:
    """one raw vbz_gpu_signal_events_batch call and its check.  starts[i]: read i's sorted event starts.  first / flat / rows: other
    tables than those of `starts` (a read whose entries differ is then expected to fail).  moments False: a NULL moments.  guard: canary
    rows behind the arenas' last row"""

    def __init__(self, fr, starts, begin=None, end=None, norm=None, stats=0, signed=True, offset=None, scale=None, first=None, flat=None, rows=None,
                 src=None, moments=True, guard=3):
        c = fr.c
        self.fr, self.starts, self.norm, self.stats, self.signed, self.guard = fr, starts, norm, stats, signed, guard
        n, dev = fr.n, c.device
        self.bg, self.en = full(begin, n), full(end, n)
        t, fl = table_and_flat(starts)
        self.table = t if first is None else np.asarray(first, np.int64)
        self.flat = fl if flat is None else flat
        self.rows = len(self.flat)
        self.out, self.mom = canaries(c, self.rows, guard)
        self.with_moments = moments
        self.result = torch.full((max(n, 1),), -8, dtype=torch.int32, device=dev)
        self.ss = torch.full((max(n, 1), 2), -777.0, dtype=torch.float32, device=dev)
        self.o = np.zeros(n, np.float32) if offset is None else np.asarray(offset, np.float32)
        self.s = np.ones(n, np.float32) if scale is None else np.asarray(scale, np.float32)
        f = fmt("f32", signed)
        self.keep = device_tables(c, f, offset, scale)
        b = c._batch(fr.src if src is None else src, fr.off, fr.size, torch.empty(0, dtype=torch.uint8, device=dev), fr.doff, fr.dcap, self.result)
        b.dst, b.dst_bytes = None, fr.dst_bytes
        ev, keep = events_struct(c, self.table, self.flat, rows)
        self.keep += keep
        m = norm[1].c_struct() if norm is not None else None
        g, keep = ranges_struct(c, begin, end, stats)
        self.keep += keep
        torch.cuda.synchronize()
        self.rc = c.L.vbz_gpu_signal_events_batch(c.ctx, ctypes.byref(b), ctypes.byref(fr.opts), int(fr.sized), ctypes.byref(f), ctypes.byref(ev),
                                                  self.out.data_ptr(), self.mom.data_ptr() if moments else None,
                                                  ctypes.byref(m) if m is not None else None, self.ss.data_ptr() if m is not None else None,
                                                  ctypes.byref(g) if (begin is not None or end is not None) else None)
        c.synchronize()
        self.err = c.L.vbz_gpu_last_error(c.ctx)

    def values(self, i):
        x = self.fr.reads[i]
        return x if self.signed else x.view(np.uint16)

    def check(self, expect=None, skip=()):
        """verdicts (expect[i]: another verdict than T x 2), every passing read's records, moments and constants, the canary elsewhere"""
        assert self.rc == 0, self.err
        fr = self.fr
        res = u32(self.result)
        got = self.out.cpu().numpy().view(np.uint32).reshape(self.rows + self.guard, 4)
        mom = self.mom.cpu().numpy().view(np.int64).reshape(self.rows + self.guard, 2)
        ss = self.ss.cpu().numpy()
        owned = np.zeros(self.rows + self.guard, bool)
        for i in range(fr.n):
            want_res = fr.T[i] * 2 if not (expect and i in expect) else expect[i]
            assert int(res[i]) == want_res, (i, hex(int(res[i])), hex(want_res))
            if i in skip:   # (rows left unspecified: a stream that failed behind the event check)
                owned[self.table[i] : self.table[i + 1]] = True
            if _lib.is_error(want_res) or i in skip:
                continue
            x = self.values(i)
            if self.norm is not None:
                want, want_mom, shift, scale = EV.norm_event_rows(x, self.bg[i], self.en[i], self.starts[i], self.norm[0], self.stats)
                assert (ss[i][0].view(np.uint32), ss[i][1].view(np.uint32)) == (shift.view(np.uint32), scale.view(np.uint32)), (
                    "shift_scale", i, fr.T[i], self.bg[i], self.en[i], ss[i], shift, scale)
            else:
                want, want_mom = EV.event_rows(x, self.bg[i], self.en[i], self.starts[i], self.o[i], self.s[i])
            lo, hi = int(self.table[i]), int(self.table[i + 1])
            assert hi - lo == len(self.starts[i]), (i, lo, hi, len(self.starts[i]))
            compare(got, mom if self.with_moments else None, lo, hi, want, want_mom, ("read", i, "T", fr.T[i], "range", self.bg[i], self.en[i]))
            owned[lo:hi] = True
        assert (got[~owned].view(np.uint8) == CANARY).all(), ("a record outside the passing reads' rows was written", np.argwhere(
            (got[~owned].view(np.uint8) != CANARY).any(axis=1))[:4].tolist())
        if self.with_moments:
            assert (mom[~owned].view(np.uint8) == CANARY).all(), "moments outside the passing reads' rows were written"
        else:
            assert (mom.view(np.uint8) == CANARY).all()
        return self


class EvCall(Call):
    """one raw vbz_gpu_pod5_signal_events_batch call over POD5 reads of several rows; starts[k]: read k's events"""

    def __init__(self, c, frames, rows, first, starts, begin=None, end=None, norm=None, stats=0, table=None, efirst=None, flat=None, **kw):
        super().__init__(c, frames, [len(x) for x in rows], PR.bounds(first, len(rows)) if table is None else table, "f32", None, norm=norm, **kw)
        self.sig = G.pod5_signals(rows, first)
        self.starts, self.stats = starts, stats
        self.bg, self.en = full(begin, len(first)), full(end, len(first))
        t, fl = table_and_flat(starts)
        self.etable = t if efirst is None else np.asarray(efirst, np.int64)
        self.flat = fl if flat is None else flat
        self.erows = len(self.flat)
        self.out, self.mom = canaries(c, self.erows, self.guard)
        self.ev, self.ekeep = events_struct(c, self.etable, self.flat)
        self.g, self.gkeep = ranges_struct(c, begin, end, stats)
        self.ranged = begin is not None or end is not None

    def call(self):
        m = ctypes.byref(self.m) if self.m is not None else None
        rc = self.c.L.vbz_gpu_pod5_signal_events_batch(self.c.ctx, ctypes.byref(self.b), ctypes.byref(self.opts), ctypes.byref(self.f),
                                                       ctypes.byref(self.reads), ctypes.byref(self.ev), self.out.data_ptr(), self.mom.data_ptr(), m,
                                                       self.ss.data_ptr() if self.m is not None else None,
                                                       ctypes.byref(self.g) if self.ranged else None)
        self.c.synchronize()
        return rc

    def check(self, norm=None, consts=None, skip=(), refused=()):
        """every read's rows against events_ref (skip: rows left unspecified; refused: rows that must still hold the canary)"""
        got = self.out.cpu().numpy().view(np.uint32).reshape(self.erows + self.guard, 4)
        mom = self.mom.cpu().numpy().view(np.int64).reshape(self.erows + self.guard, 2)
        ss = self.ss.cpu().numpy()
        owned = np.zeros(self.erows + self.guard, bool)
        for k, x in enumerate(self.sig):
            lo, hi = int(self.etable[k]), int(self.etable[k + 1])
            if k in skip:
                owned[lo:hi] = True
            if k in skip or k in refused:
                continue
            if norm is not None:
                want, want_mom, shift, scale = EV.norm_event_rows(x, self.bg[k], self.en[k], self.starts[k], norm, self.stats)
                assert (ss[k][0].view(np.uint32), ss[k][1].view(np.uint32)) == (shift.view(np.uint32), scale.view(np.uint32)), ("shift_scale", k)
            else:
                want, want_mom = EV.event_rows(x, self.bg[k], self.en[k], self.starts[k], consts[k][0], consts[k][1])
            compare(got, mom, lo, hi, want, want_mom, ("read", k, "T", len(x), "range", self.bg[k], self.en[k]))
            owned[lo:hi] = True
        assert (got[~owned].view(np.uint8) == CANARY).all(), "a record outside the passing reads' rows was written"
        assert (mom[~owned].view(np.uint8) == CANARY).all(), "moments outside the passing reads' rows were written"
