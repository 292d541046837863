"""The raw span calls for the signal-span tests on the MI355X (test_gpu_spans, test_gpu_spans_refusals): one call into canary tables
(segment_support.Tables: edge_first with guard entries behind it, edge with guard entries in front of and behind its edge_cap entries,
shift_scale and level canaried too), and its check, bit for bit, against spans_ref -- over reads (typed_support.Frames) and over POD5
reads of several rows (typed_support.Call).  A plain module: every assert carries its operands."""
import ctypes

import numpy as np
import torch

import norm_ref as R
import pod5_reads_ref as PR
import ranges_ref as G
import spans_ref as S
from segment_support import E_DEST, Tables
from typed_support import Call, full, ranges_struct, u32
from vbz_compression_amd import _lib

SS_CANARY = -777.0


def span_struct(P, edge_cap, level=None, flags=0):
    g = _lib.GpuSpans()
    g.direction, g.merge_gap, g.min_length, g.ignore_prefix, g.threshold_factor = P
    g.flags, g.edge_cap = flags, edge_cap
    g.level = level.data_ptr() if level is not None else None
    return g


def norm_levels(signals, bg, en, p, stats):
    """{shift, scale} of every read as the statistics-alone call gives them (ranges_ref: over the range, or over the read with stats 1)"""
    out = []
    for i, x in enumerate(signals):
        b, e = G.clamp(len(x), bg[i], en[i])
        v = x if stats == 1 else x[b:e]
        out.append(R.shift_scale(v, p))
    return out


def level_table(c, levels, n):
    """float32 [n + 1, 2] on the device: the reads' {a, w} and a canary row behind them"""
    t = np.full((n + 1, 2), SS_CANARY, np.float32)
    for i, (a, w) in enumerate(levels):
        t[i] = (a, w)
    return torch.from_numpy(t).to(c.device)


class SpanRun:
    """one raw vbz_gpu_signal_spans_batch call and its check.  levels: per read (a, w) -- the given constants; norm: (norm_ref's tuple,
    batch.Normalization) instead.  cap: edge_cap (None: exactly the total); count_only: edge NULL"""

    def __init__(self, fr, P=S.DEFAULT, levels=None, norm=None, begin=None, end=None, stats=0, signed=True, cap=None, count_only=False, src=None,
                 failed=(), guard=4, with_ss=True):
        c = fr.c
        self.fr, self.P, self.signed, self.failed, self.norm = fr, P, signed, set(failed), norm
        n = fr.n
        self.bg, self.en = full(begin, n), full(end, n)
        sig = [self.values(i) for i in range(n)]
        self.levels = levels if norm is None else norm_levels(sig, self.bg, self.en, norm[0], stats)
        self.want_first, self.want_ed = S.tables(sig, P, self.levels, self.bg, self.en, self.failed)
        self.t = Tables(c, n, int(self.want_first[-1]), cap, count_only, guard)
        self.result = torch.full((max(n, 1),), -8, dtype=torch.int32, device=c.device)
        self.ss = torch.full((n + 1, 2), SS_CANARY, dtype=torch.float32, device=c.device)
        self.level = level_table(c, self.levels, n) if norm is None else None
        b = c._batch(fr.src if src is None else src, fr.off, fr.size, torch.empty(0, dtype=torch.uint8, device=c.device), fr.doff, fr.dcap, self.result)
        b.dst, b.dst_bytes = None, fr.dst_bytes
        g, self.keep = ranges_struct(c, begin, end, stats)
        sp = span_struct(P, self.t.cap, self.level)
        m = norm[1].c_struct() if norm is not None else None
        torch.cuda.synchronize()
        self.rc = c.L.vbz_gpu_signal_spans_batch(c.ctx, ctypes.byref(b), ctypes.byref(fr.opts), int(fr.sized), int(signed),
                                                 ctypes.byref(m) if m is not None else None, self.ss.data_ptr() if (m is not None and with_ss) else None,
                                                 ctypes.byref(g) if (begin is not None or end is not None) else None, ctypes.byref(sp),
                                                 self.t.first.data_ptr(), self.t.start_ptr)
        c.synchronize()
        self.err = c.L.vbz_gpu_last_error(c.ctx)
        self.with_ss = with_ss and m is not None

    def values(self, i):
        x = self.fr.reads[i]
        return x if self.signed else x.view(np.uint16)

    def check(self, expect=None, spans_min=1):
        """verdicts (expect[i]: another verdict than T x 2 -- such a read must be in `failed`), the tables, shift_scale, the canaries; the
        reference lists at least spans_min spans in all (a case cannot pass on empty tables)"""
        assert self.rc == 0, self.err
        fr = self.fr
        assert int(self.want_first[-1]) >= 2 * spans_min, ("the reference lists too few spans", self.P, int(self.want_first[-1]) // 2, spans_min)
        refused = self.t.check(fr.n, self.want_first, self.want_ed, (self.P, "T", fr.T[:8]))
        res = u32(self.result)
        for i in range(fr.n):
            want = E_DEST if i in refused else (fr.T[i] * 2 if not (expect and i in expect) else expect[i])
            assert int(res[i]) == want, (i, hex(int(res[i])), hex(want))
            assert (i in self.failed) == (_lib.is_error(want) and i not in refused), i
        ss = self.ss.cpu().numpy()
        if self.with_ss:
            for i in range(fr.n):
                if i in self.failed:
                    continue
                a, w = self.levels[i]
                assert (ss[i][0].view(np.uint32), ss[i][1].view(np.uint32)) == (np.float32(a).view(np.uint32), np.float32(w).view(np.uint32)), (
                    "shift_scale", i, ss[i], a, w)
            assert (ss[fr.n] == SS_CANARY).all(), "shift_scale behind its last read was written"
        else:
            assert (ss == SS_CANARY).all(), "shift_scale was written"
        if self.level is not None:
            assert (self.level.cpu().numpy()[fr.n] == SS_CANARY).all()
        self.refused = refused
        return self

    def tables_bytes(self):
        return self.t.first.cpu().numpy().tobytes(), self.t.start.cpu().numpy().tobytes(), u32(self.result).tolist()


class SpanCall(Call):
    """one raw vbz_gpu_pod5_signal_spans_batch call over POD5 reads of several rows"""

    def __init__(self, c, frames, rows, first, P=S.DEFAULT, levels=None, norm=None, begin=None, end=None, stats=0, signed=True, cap=None,
                 count_only=False, table=None, failed=(), **kw):
        super().__init__(c, frames, [len(x) for x in rows], PR.bounds(first, len(rows)) if table is None else table, "f32", None, signed=signed, **kw)
        self.P, self.signed, self.failed = P, signed, set(failed)
        sig = G.pod5_signals(rows, first)
        self.sig = sig if signed else [np.asarray(x).view(np.uint16) for x in sig]
        self.bounds = PR.bounds(first, len(rows))
        self.row_len = [len(x) for x in rows]
        n = len(first)
        self.bg, self.en = full(begin, n), full(end, n)
        self.levels = levels if norm is None else norm_levels(self.sig, self.bg, self.en, norm[0], stats)
        self.want_first, self.want_ed = S.tables(self.sig, P, self.levels, self.bg, self.en, self.failed)
        self.t = Tables(c, n, int(self.want_first[-1]), cap, count_only, self.guard)
        self.g, self.gkeep = ranges_struct(c, begin, end, stats)
        self.ranged = begin is not None or end is not None
        self.level = level_table(c, self.levels, n) if norm is None else None
        self.sp = span_struct(P, self.t.cap, self.level)
        self.nm = norm[1].c_struct() if norm is not None else None
        self.ss2 = torch.full((n + 1, 2), SS_CANARY, dtype=torch.float32, device=c.device)

    def call(self):
        rc = self.c.L.vbz_gpu_pod5_signal_spans_batch(self.c.ctx, ctypes.byref(self.b), ctypes.byref(self.opts), int(self.signed), ctypes.byref(self.reads),
                                                      ctypes.byref(self.nm) if self.nm is not None else None,
                                                      self.ss2.data_ptr() if self.nm is not None else None, ctypes.byref(self.g) if self.ranged else None,
                                                      ctypes.byref(self.sp), self.t.first.data_ptr(), self.t.start_ptr)
        self.c.synchronize()
        return rc

    def check(self, row_expect=None, spans_min=1):
        """the tables; the rows' and the reads' verdicts (row_expect[j]: another verdict of row j than its samples x 2; a read that does not
        fit the cap has E_DEST on every row); shift_scale with a normalisation"""
        assert int(self.want_first[-1]) >= 2 * spans_min, ("the reference lists too few spans", int(self.want_first[-1]) // 2)
        refused = self.t.check(self.R, self.want_first, self.want_ed, (self.P, "pod5"))
        res, rres = u32(self.result)[: self.n].tolist(), u32(self.read_result)[: self.R].tolist()
        for k in range(self.R):
            rows = range(self.bounds[k], self.bounds[k + 1])
            want = [E_DEST if k in refused else (2 * self.row_len[j] if not (row_expect and j in row_expect) else row_expect[j]) for j in rows]
            assert [res[j] for j in rows] == want, ("read", k, [hex(res[j]) for j in rows], [hex(v) for v in want])
            bad = [v for v in want if _lib.is_error(v)]
            assert rres[k] == (bad[0] if bad else 2 * len(self.sig[k])), ("read_result", k, hex(rres[k]))
        ss = self.ss2.cpu().numpy()
        if self.nm is not None:
            for k in range(self.R):
                if k in self.failed:
                    continue
                a, w = self.levels[k]
                assert (ss[k][0].view(np.uint32), ss[k][1].view(np.uint32)) == (np.float32(a).view(np.uint32), np.float32(w).view(np.uint32)), ("shift_scale", k)
        assert (ss[self.R] == SS_CANARY).all()
        self.refused = refused
        return self
