"""The raw span calls for the signal-match tests that also take the start (test_gpu_match_span, test_gpu_match_span_refusals): what
match_support is to the cost-only calls.  The stage entry over one call of a catalogue into a canary-filled arena of 16-byte hits with a
guard row behind it, and the fused calls over reads (typed_support.Frames) and over POD5 reads (typed_support.Call), checked bit for bit
against windows_ref (the query) and match_span_ref (the spans of that query)."""
import ctypes

import numpy as np
import torch

import match_span_ref as S
import pod5_reads_ref as PR
import ranges_ref as G
from match_support import HIT_CANARY, Q_CANARY, SS_CANARY, Arenas, assert_hits, match_struct, query_rows
from typed_support import Call, device_tables, fmt, full, i32, ranges_struct, u32
from vbz_compression_amd import _lib

EMPTY = [0xFFFFFFFF, 0, 0, 0]


def stage_span(c, call, cost_only=False):
    """vbz_gpu_match_span_batch over one call of a catalogue -> uint32 [reads, R, 4] (cost_only: vbz_gpu_match_batch, [reads, R, 2]); the
    guard row behind the hits keeps its canary and the query its bits"""
    query, valid, ref, ref_len = call.arrays()
    n, R, words = len(query), len(ref), 2 if cost_only else 4
    m, keep = match_struct(c, call.N, call.quant, ref, ref_len)
    q = torch.from_numpy(query).to(c.device)
    v = i32(valid).to(c.device)
    out = torch.full((n + 1, R, words), HIT_CANARY, dtype=torch.int32, device=c.device)
    torch.cuda.synchronize()
    fn = c.L.vbz_gpu_match_batch if cost_only else c.L.vbz_gpu_match_span_batch
    rc = fn(c.ctx, n, q.data_ptr(), v.data_ptr(), ctypes.byref(m), out.data_ptr())
    c.synchronize()
    assert rc == 0, c.L.vbz_gpu_last_error(c.ctx)
    got = out.cpu().numpy().view(np.uint32)
    assert (got[n] == HIT_CANARY).all(), "hits behind the last read were written"
    assert (q.cpu().numpy().view(np.uint32) == query.view(np.uint32)).all(), "the stage entry wrote its query"
    return got[:n]


class SpanArenas(Arenas):
    """canary-filled query, 16-byte hits and shift_scale of n reads, a guard row behind each"""

    def __init__(self, c, n, N, R):
        super().__init__(c, n, N, R)
        self.out = torch.full((n + 1, R, 4), HIT_CANARY, dtype=torch.int32, device=c.device)

    def check(self, want_q, want_ss, Tp, quant, ref, ref_len, failed, what):
        """as Arenas.check, the hits against match_span_ref"""
        n, N = self.n, self.N
        q = self.query.cpu().numpy()
        ok = [i for i in range(n) if i not in failed]
        bad = np.argwhere(q.view(np.uint32)[ok] != want_q[ok])
        assert bad.size == 0, (what, "query: read (among the passing), position", bad[:4].tolist())
        assert (q[n] == Q_CANARY).all(), "the query row behind the last read was written"
        valid = [0 if i in failed else min(Tp[i], N) for i in range(n)]
        want = S.spans(want_q.view(np.float32), valid, quant, ref, ref_len)
        got = self.out.cpu().numpy().view(np.uint32)
        assert_hits(got[:n], want, what)
        assert (got[n] == HIT_CANARY).all(), "hits behind the last read were written"
        for i in failed:
            assert got[i].tolist() == [EMPTY] * self.R, (what, "failed read", i)
        ss = self.ss.cpu().numpy()
        if want_ss:
            for i in ok:
                assert (ss[i][0].view(np.uint32), ss[i][1].view(np.uint32)) == (want_ss[i][0].view(np.uint32), want_ss[i][1].view(np.uint32)), ("shift_scale", i)
            assert (ss[n] == SS_CANARY).all()
        else:
            assert (ss == SS_CANARY).all(), "shift_scale was written"
        return want


class SpanRun:
    """one raw vbz_gpu_signal_match_span_batch call and its check (match_support.MatchRun's arguments)"""

    def __init__(self, fr, ref, ref_len, N, quant=32.0, begin=None, end=None, norm=None, stats=0, signed=True, offset=None, scale=None, src=None):
        c = fr.c
        self.fr, self.ref, self.ref_len, self.N, self.quant, self.norm, self.stats, self.signed = fr, ref, ref_len, N, quant, norm, stats, signed
        n, dev = fr.n, c.device
        self.bg, self.en = full(begin, n), full(end, n)
        self.a = SpanArenas(c, n, N, len(ref))
        self.result = torch.full((max(n, 1),), -8, dtype=torch.int32, device=dev)
        self.o = np.zeros(n, np.float32) if offset is None else np.asarray(offset, np.float32)
        self.s = np.ones(n, np.float32) if scale is None else np.asarray(scale, np.float32)
        f = fmt("f32", signed)
        self.keep = device_tables(c, f, offset, scale)
        b = c._batch(fr.src if src is None else src, fr.off, fr.size, torch.empty(0, dtype=torch.uint8, device=dev), fr.doff, fr.dcap, self.result)
        b.dst, b.dst_bytes = None, fr.dst_bytes
        mt, keep = match_struct(c, N, quant, ref, ref_len)
        self.keep += keep
        m = norm[1].c_struct() if norm is not None else None
        g, keep = ranges_struct(c, begin, end, stats)
        self.keep += keep
        torch.cuda.synchronize()
        self.rc = c.L.vbz_gpu_signal_match_span_batch(c.ctx, ctypes.byref(b), ctypes.byref(fr.opts), int(fr.sized), ctypes.byref(f),
                                                      ctypes.byref(m) if m is not None else None, self.a.ss.data_ptr() if m is not None else None,
                                                      ctypes.byref(g) if (begin is not None or end is not None) else None, ctypes.byref(mt),
                                                      self.a.query.data_ptr(), self.a.out.data_ptr())
        c.synchronize()
        self.err = c.L.vbz_gpu_last_error(c.ctx)

    def check(self, expect=None):
        """verdicts (expect[i]: another verdict than T x 4 -- an error: the read's hits are the empty verdict), the query, the spans"""
        assert self.rc == 0, self.err
        fr = self.fr
        res = u32(self.result)
        failed = set()
        for i in range(fr.n):
            want = fr.T[i] * 4 if not (expect and i in expect) else expect[i]
            assert int(res[i]) == want, (i, hex(int(res[i])), hex(want))
            if _lib.is_error(want):
                failed.add(i)
        sig = [x if self.signed else x.view(np.uint16) for x in fr.reads]
        want_q, want_ss, Tp = query_rows(sig, self.bg, self.en, self.N, list(zip(self.o, self.s)), self.norm[0] if self.norm else None, self.stats)
        self.want = self.a.check(want_q, want_ss, Tp, self.quant, self.ref, self.ref_len, failed, ("N", self.N, "T", fr.T[:8]))
        return self


class SpanCall(Call):
    """one raw vbz_gpu_pod5_signal_match_span_batch call over POD5 reads of several rows (match_support.MatchCall's arguments)"""

    def __init__(self, c, frames, rows, first, ref, ref_len, N, quant=32.0, begin=None, end=None, norm=None, stats=0, table=None, **kw):
        super().__init__(c, frames, [len(x) for x in rows], PR.bounds(first, len(rows)) if table is None else table, "f32", None, norm=norm, **kw)
        self.sig = G.pod5_signals(rows, first)
        self.ref, self.ref_len, self.N, self.quant, self.stats = ref, ref_len, N, quant, stats
        n = len(first)
        self.bg, self.en = full(begin, n), full(end, n)
        self.a = SpanArenas(c, n, N, len(ref))
        self.mt, self.mkeep = match_struct(c, N, quant, ref, ref_len)
        self.g, self.gkeep = ranges_struct(c, begin, end, stats)
        self.ranged = begin is not None or end is not None

    def call(self, read_result=True):
        if not read_result:
            self.reads.read_result = None
        m = ctypes.byref(self.m) if self.m is not None else None
        rc = self.c.L.vbz_gpu_pod5_signal_match_span_batch(self.c.ctx, ctypes.byref(self.b), ctypes.byref(self.opts), ctypes.byref(self.f),
                                                           ctypes.byref(self.reads), m, self.a.ss.data_ptr() if self.m is not None else None,
                                                           ctypes.byref(self.g) if self.ranged else None, ctypes.byref(self.mt), self.a.query.data_ptr(),
                                                           self.a.out.data_ptr())
        self.c.synchronize()
        return rc

    def check(self, norm=None, consts=None, failed=()):
        want_q, want_ss, Tp = query_rows(self.sig, self.bg, self.en, self.N, consts, norm, self.stats)
        self.want = self.a.check(want_q, want_ss, Tp, self.quant, self.ref, self.ref_len, set(failed), ("pod5", "N", self.N))
        return self
