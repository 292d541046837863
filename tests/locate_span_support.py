"""The raw locate span calls for the tests on the MI355X (test_gpu_locate_span, test_gpu_locate_span_refusals): what locate_support is to
the cost-only calls.  The stage entry into a canary-filled arena of 16-byte hits with a guard row behind it, the same cells through
vbz_gpu_match_span_batch with the roles swapped, and the fused calls -- over reads (typed_support.Frames) and over POD5 reads of several
rows (typed_support.Call) -- checked bit for bit against windows_ref (the query) and locate_span_ref (the spans of that query)."""
import ctypes

import numpy as np
import torch

import locate_span_ref as LS
import match_ref as M
import pod5_reads_ref as PR
import ranges_ref as G
from locate_support import locate_struct
from match_support import HIT_CANARY, Q_CANARY, SS_CANARY, Arenas, assert_hits, match_struct, query_rows
from typed_support import Call, device_tables, fmt, full, i32, ranges_struct, u32
from vbz_compression_amd import _lib

EMPTY = [0xFFFFFFFF, 0, 0, 0]


def stage_arrays(c, query, valid, quant, target, target_len, cost_only=False, keep_out=False):
    """vbz_gpu_locate_span_batch -> uint32 [reads, G, 4] (cost_only: vbz_gpu_locate_batch, [reads, G, 2]); the guard row behind the hits
    keeps its canary, the query arena is left unwritten.  keep_out: also the device arena of the reads' hits, for a call queued behind"""
    n, Gn, N, words = len(query), len(target), query.shape[1], 2 if cost_only else 4
    m, keep = locate_struct(c, N, quant, target, target_len)
    q = torch.from_numpy(np.array(query, np.float32)).to(c.device)
    v = i32(valid).to(c.device)
    out = torch.full((n + 1, Gn, words), HIT_CANARY, dtype=torch.int32, device=c.device)
    torch.cuda.synchronize()
    fn = c.L.vbz_gpu_locate_batch if cost_only else c.L.vbz_gpu_locate_span_batch
    rc = fn(c.ctx, n, q.data_ptr(), v.data_ptr(), ctypes.byref(m), out.data_ptr())
    c.synchronize()
    assert rc == 0, c.L.vbz_gpu_last_error(c.ctx)
    got = out.cpu().numpy().view(np.uint32)
    assert (got[n] == HIT_CANARY).all(), "hits behind the last read were written"
    assert (q.cpu().numpy().view(np.uint32) == np.ascontiguousarray(query).view(np.uint32)).all(), "the stage entry wrote its query"
    return (got[:n], out) if keep_out else got[:n]


def stage(c, call, **kw):
    query, valid, target, target_len = call.arrays()
    return stage_arrays(c, query, valid, call.quant, target, target_len, **kw)


def swapped_match_span(c, query, valid, quant, target, target_len):
    """the same cells through vbz_gpu_match_span_batch with the roles swapped (locate_support.swapped_match's construction: targets of at
    most 65 536 levels and without -128, written out as float32 "queries"; the reads' levels as int8 "references") -> uint32 [reads, G, 4].
    The match rule's query limit decides packed or wide by itself."""
    N, stride = query.shape[1], target.shape[1]
    assert stride <= 65536 and stride % 8 == 0 and N % 16 == 0
    L = np.asarray(target_len, np.uint64)
    tvalid = np.where((L != 0) & (L <= stride), L, 0).astype(np.uint32)
    tq = np.asarray(target, np.float32) / np.float32(quant)
    levels = M.quantize(query, quant)
    n = np.minimum(np.asarray(valid, np.uint64), N).astype(np.uint32)
    m, keep = match_struct(c, stride, quant, levels, n)
    q = torch.from_numpy(np.ascontiguousarray(tq)).to(c.device)
    v = i32(tvalid).to(c.device)
    out = torch.full((len(target), len(query), 4), HIT_CANARY, dtype=torch.int32, device=c.device)
    torch.cuda.synchronize()
    rc = c.L.vbz_gpu_match_span_batch(c.ctx, len(target), q.data_ptr(), v.data_ptr(), ctypes.byref(m), out.data_ptr())
    c.synchronize()
    assert rc == 0, c.L.vbz_gpu_last_error(c.ctx)
    return np.ascontiguousarray(out.cpu().numpy().view(np.uint32).transpose(1, 0, 2))


class SpanArenas(Arenas):
    """canary-filled query, 16-byte hits and shift_scale of n reads, a guard row behind each"""

    def __init__(self, c, n, N, Gn):
        super().__init__(c, n, N, Gn)
        self.out = torch.full((n + 1, Gn, 4), HIT_CANARY, dtype=torch.int32, device=c.device)

    def check(self, want_q, want_ss, Tp, quant, target, target_len, failed, what):
        """as locate_support.LocateArenas.check, the hits against locate_span_ref"""
        n, N = self.n, self.N
        q = self.query.cpu().numpy()
        ok = [i for i in range(n) if i not in failed]
        bad = np.argwhere(q.view(np.uint32)[ok] != want_q[ok])
        assert bad.size == 0, (what, "query: read (among the passing), position", bad[:4].tolist())
        assert (q[n] == Q_CANARY).all(), "the query row behind the last read was written"
        valid = [0 if i in failed else min(Tp[i], N) for i in range(n)]
        want = LS.spans(want_q.view(np.float32), valid, quant, target, target_len)
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
    """one raw vbz_gpu_signal_locate_span_batch call and its check (locate_support.LocateRun's arguments)"""

    def __init__(self, fr, target, target_len, N, quant=32.0, begin=None, end=None, norm=None, stats=0, signed=True, offset=None, scale=None, src=None):
        c = fr.c
        self.fr, self.target, self.target_len, self.N, self.quant, self.norm, self.stats, self.signed = fr, target, target_len, N, quant, norm, stats, signed
        n, dev = fr.n, c.device
        self.bg, self.en = full(begin, n), full(end, n)
        self.a = SpanArenas(c, n, N, len(target))
        self.result = torch.full((max(n, 1),), -8, dtype=torch.int32, device=dev)
        self.o = np.zeros(n, np.float32) if offset is None else np.asarray(offset, np.float32)
        self.s = np.ones(n, np.float32) if scale is None else np.asarray(scale, np.float32)
        f = fmt("f32", signed)
        self.keep = device_tables(c, f, offset, scale)
        b = c._batch(fr.src if src is None else src, fr.off, fr.size, torch.empty(0, dtype=torch.uint8, device=dev), fr.doff, fr.dcap, self.result)
        b.dst, b.dst_bytes = None, fr.dst_bytes
        lc, keep = locate_struct(c, N, quant, target, target_len)
        self.keep += keep
        m = norm[1].c_struct() if norm is not None else None
        g, keep = ranges_struct(c, begin, end, stats)
        self.keep += keep
        torch.cuda.synchronize()
        self.rc = c.L.vbz_gpu_signal_locate_span_batch(c.ctx, ctypes.byref(b), ctypes.byref(fr.opts), int(fr.sized), ctypes.byref(f),
                                                       ctypes.byref(m) if m is not None else None, self.a.ss.data_ptr() if m is not None else None,
                                                       ctypes.byref(g) if (begin is not None or end is not None) else None, ctypes.byref(lc),
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
        self.want = self.a.check(want_q, want_ss, Tp, self.quant, self.target, self.target_len, failed, ("N", self.N, "T", fr.T[:8]))
        return self


class SpanCall(Call):
    """one raw vbz_gpu_pod5_signal_locate_span_batch call over POD5 reads of several rows (locate_support.LocateCall's arguments)"""

    def __init__(self, c, frames, rows, first, target, target_len, N, quant=32.0, begin=None, end=None, norm=None, stats=0, table=None, **kw):
        super().__init__(c, frames, [len(x) for x in rows], PR.bounds(first, len(rows)) if table is None else table, "f32", None, norm=norm, **kw)
        self.sig = G.pod5_signals(rows, first)
        self.target, self.target_len, self.N, self.quant, self.stats = target, target_len, N, quant, stats
        n = len(first)
        self.bg, self.en = full(begin, n), full(end, n)
        self.a = SpanArenas(c, n, N, len(target))
        self.lc, self.lkeep = locate_struct(c, N, quant, target, target_len)
        self.g, self.gkeep = ranges_struct(c, begin, end, stats)
        self.ranged = begin is not None or end is not None

    def call(self, read_result=True):
        if not read_result:
            self.reads.read_result = None
        m = ctypes.byref(self.m) if self.m is not None else None
        rc = self.c.L.vbz_gpu_pod5_signal_locate_span_batch(self.c.ctx, ctypes.byref(self.b), ctypes.byref(self.opts), ctypes.byref(self.f),
                                                            ctypes.byref(self.reads), m, self.a.ss.data_ptr() if self.m is not None else None,
                                                            ctypes.byref(self.g) if self.ranged else None, ctypes.byref(self.lc),
                                                            self.a.query.data_ptr(), self.a.out.data_ptr())
        self.c.synchronize()
        return rc

    def check(self, norm=None, consts=None, failed=()):
        want_q, want_ss, Tp = query_rows(self.sig, self.bg, self.en, self.N, consts, norm, self.stats)
        self.want = self.a.check(want_q, want_ss, Tp, self.quant, self.target, self.target_len, set(failed), ("pod5", "N", self.N))
        return self
