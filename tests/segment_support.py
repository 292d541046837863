"""The raw segmentation calls for the signal-segmentation tests on the MI355X (test_gpu_segment, test_gpu_segment_refusals): one call into
canary tables (event_first with guard entries behind it, start with guard entries in front of and behind its start_cap entries), and its
check, bit for bit, against segment_ref -- over reads (typed_support.Frames) and over POD5 reads of several rows (typed_support.Call).  A
plain module: every assert carries its operands."""
import ctypes

import numpy as np
import torch

import pod5_reads_ref as PR
import ranges_ref as G
import segment_ref as S
from typed_support import Call, full, ranges_struct, u32
from vbz_compression_amd import _lib

CANARY32 = 0x5A5A5A5A
CANARY64 = 0x5A5A5A5A5A5A5A5A
E_DEST = 0xFFFFFFFC
LEAD = 3   # canary entries in front of start[0]


def seg_struct(P, start_cap, flags=0):
    g = _lib.GpuSegmentation()
    g.short_window, g.long_window, g.short_threshold, g.long_threshold, g.radius = P
    g.flags, g.start_cap = flags, start_cap
    return g


def expected(signals, bg, en, P, failed=()):
    """(event_first, the reads' starts) the call must write: segment_ref's, a read in `failed` (an error verdict) owning no row"""
    st = [np.zeros(0, np.uint32) if i in failed else S.starts(x, bg[i], en[i], P) for i, x in enumerate(signals)]
    return np.concatenate([[0], np.cumsum([len(v) for v in st])]).astype(np.int64), st


class Tables:
    """the two output tables of a call over n reads, canary-filled: cap None -> the exact total `total`; count_only: no start at all"""

    def __init__(self, c, n, total, cap, count_only, guard):
        self.cap = 0 if count_only else (total if cap is None else cap)
        self.guard, self.count_only = guard, count_only
        self.first = torch.full((n + 1 + guard,), CANARY64, dtype=torch.int64, device=c.device)
        self.start = torch.full((LEAD + self.cap + guard,), CANARY32, dtype=torch.int32, device=c.device)
        self.start_ptr = None if count_only else self.start.data_ptr() + 4 * LEAD

    def check(self, n, want_first, want_st, what):
        """event_first complete whatever the cap; the starts of exactly the reads whose rows end at or in front of the cap; the canary
        everywhere else.  Returns the reads that did not fit"""
        first = self.first.cpu().numpy()
        assert first[: n + 1].tolist() == want_first.tolist(), (what, "event_first", first[: n + 1].tolist()[:12], want_first.tolist()[:12])
        assert (first[n + 1 :] == CANARY64).all(), (what, "entries behind event_first[n] were written")
        got = u32(self.start)
        owned = np.zeros(len(got), bool)
        refused = set()
        for i in range(n):
            lo, hi = int(want_first[i]), int(want_first[i + 1])
            if self.count_only or lo == hi:
                continue
            if hi > self.cap:
                refused.add(i)
                continue
            assert got[LEAD + lo : LEAD + hi].tolist() == want_st[i].tolist(), (what, "read", i, "rows", lo, hi, got[LEAD + lo : LEAD + hi].tolist()[:12],
                                                                                 want_st[i].tolist()[:12])
            owned[LEAD + lo : LEAD + hi] = True
        assert (got[~owned] == CANARY32).all(), (what, "an entry of start owned by no fitting read was written", np.flatnonzero(got[~owned] != CANARY32)[:8].tolist())
        return refused


class SegRun:
    """one raw vbz_gpu_signal_segment_batch call and its check.  cap: start_cap (None: exactly the total); count_only: start NULL"""

    def __init__(self, fr, P=S.DEFAULT, begin=None, end=None, signed=True, cap=None, count_only=False, src=None, failed=(), guard=4):
        c = fr.c
        self.fr, self.P, self.signed, self.failed = fr, P, signed, set(failed)
        n = fr.n
        self.bg, self.en = full(begin, n), full(end, n)
        self.want_first, self.want_st = expected([self.values(i) for i in range(n)], self.bg, self.en, P, self.failed)
        self.t = Tables(c, n, int(self.want_first[-1]), cap, count_only, guard)
        self.result = torch.full((max(n, 1),), -8, dtype=torch.int32, device=c.device)
        b = c._batch(fr.src if src is None else src, fr.off, fr.size, torch.empty(0, dtype=torch.uint8, device=c.device), fr.doff, fr.dcap, self.result)
        b.dst, b.dst_bytes = None, fr.dst_bytes
        g, self.keep = ranges_struct(c, begin, end)
        sg = seg_struct(P, self.t.cap)
        torch.cuda.synchronize()
        self.rc = c.L.vbz_gpu_signal_segment_batch(c.ctx, ctypes.byref(b), ctypes.byref(fr.opts), int(fr.sized), int(signed),
                                                   ctypes.byref(g) if (begin is not None or end is not None) else None, ctypes.byref(sg),
                                                   self.t.first.data_ptr(), self.t.start_ptr)
        c.synchronize()
        self.err = c.L.vbz_gpu_last_error(c.ctx)

    def values(self, i):
        x = self.fr.reads[i]
        return x if self.signed else x.view(np.uint16)

    def check(self, expect=None, rows_min=2):
        """verdicts (expect[i]: another verdict than T x 2 -- such a read must be in `failed`), the tables, the canaries; the reference
        lists at least rows_min rows for some read (a case cannot pass vacuously)"""
        assert self.rc == 0, self.err
        fr = self.fr
        assert max([len(v) for v in self.want_st] + [0]) >= rows_min, ("the reference lists no boundary", [len(v) for v in self.want_st][:8])
        refused = self.t.check(fr.n, self.want_first, self.want_st, (self.P, "T", fr.T[:8]))
        res = u32(self.result)
        for i in range(fr.n):
            want = E_DEST if i in refused else (fr.T[i] * 2 if not (expect and i in expect) else expect[i])
            assert int(res[i]) == want, (i, hex(int(res[i])), hex(want))
            assert (i in self.failed) == (_lib.is_error(want) and i not in refused), i
        self.refused = refused
        return self


class SegCall(Call):
    """one raw vbz_gpu_pod5_signal_segment_batch call over POD5 reads of several rows"""

    def __init__(self, c, frames, rows, first, P=S.DEFAULT, begin=None, end=None, signed=True, cap=None, count_only=False, table=None, failed=(), **kw):
        super().__init__(c, frames, [len(x) for x in rows], PR.bounds(first, len(rows)) if table is None else table, "f32", None, signed=signed, **kw)
        self.P, self.signed, self.failed = P, signed, set(failed)
        sig = G.pod5_signals(rows, first)
        self.sig = sig if signed else [np.asarray(x).view(np.uint16) for x in sig]
        self.bounds = PR.bounds(first, len(rows))
        self.row_len = [len(x) for x in rows]
        R = len(first)
        self.bg, self.en = full(begin, R), full(end, R)
        self.want_first, self.want_st = expected(self.sig, self.bg, self.en, P, self.failed)
        self.t = Tables(c, R, int(self.want_first[-1]), cap, count_only, self.guard)
        self.g, self.gkeep = ranges_struct(c, begin, end)
        self.ranged = begin is not None or end is not None
        self.sg = seg_struct(P, self.t.cap)

    def call(self):
        rc = self.c.L.vbz_gpu_pod5_signal_segment_batch(self.c.ctx, ctypes.byref(self.b), ctypes.byref(self.opts), int(self.signed), ctypes.byref(self.reads),
                                                        ctypes.byref(self.g) if self.ranged else None, ctypes.byref(self.sg), self.t.first.data_ptr(),
                                                        self.t.start_ptr)
        self.c.synchronize()
        return rc

    def check(self, row_expect=None, rows_min=2):
        """the tables; the rows' and the reads' verdicts (row_expect[j]: another verdict of row j than its samples x 2; a read that does not
        fit the cap has E_DEST on every row)"""
        assert max([len(v) for v in self.want_st] + [0]) >= rows_min, "the reference lists no boundary"
        refused = self.t.check(self.R, self.want_first, self.want_st, (self.P, "pod5"))
        res, rres = u32(self.result)[: self.n].tolist(), u32(self.read_result)[: self.R].tolist()
        for k in range(self.R):
            rows = range(self.bounds[k], self.bounds[k + 1])
            want = [E_DEST if k in refused else (2 * self.row_len[j] if not (row_expect and j in row_expect) else row_expect[j]) for j in rows]
            assert [res[j] for j in rows] == want, ("read", k, [hex(res[j]) for j in rows], [hex(v) for v in want])
            bad = [v for v in want if _lib.is_error(v)]
            assert rres[k] == (bad[0] if bad else 2 * len(self.sig[k])), ("read_result", k, hex(rres[k]))
        self.refused = refused
        return self
