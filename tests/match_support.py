"""The raw match calls for the signal-match tests on the MI355X (test_gpu_match, test_gpu_match_refusals): the stage entry over one call
of match_ref's catalogue, and the fused calls -- over reads (typed_support.Frames) and over POD5 reads of several rows
(typed_support.Call) -- into canary-filled query, hit and shift_scale arenas with a guard row behind each, checked bit for bit against
windows_ref (the query) and match_ref (the hits of that query).  A plain module: every assert carries its operands."""
import ctypes

import numpy as np
import torch

import match_ref as M
import pod5_reads_ref as PR
import ranges_ref as G
import windows_ref as W
from typed_support import Call, device_tables, fmt, full, i32, ranges_struct, u32
from vbz_compression_amd import _lib

Q_CANARY = -555.0          # the query arena's fill (a float: its bits are compared)
HIT_CANARY = 0x5A5A5A5A    # every word of the hit arena
SS_CANARY = -777.0
EMPTY = [0xFFFFFFFF, 0]


def match_struct(c, N, quant, ref, ref_len, flags=0, reserved=0):
    """(vbz_gpu_match, its tables): ref int8 [R, stride], ref_len any integers 0 ... 2^32 - 1"""
    ref_d = torch.from_numpy(np.ascontiguousarray(ref, np.int8)).to(c.device)
    len_d = i32(ref_len).to(c.device)
    m = _lib.GpuMatch()
    m.query_len, m.n_refs, m.ref_stride, m.flags, m.quant, m.reserved = N, ref.shape[0], ref.shape[1], flags, quant, reserved
    m.ref, m.ref_len = ref_d.data_ptr(), len_d.data_ptr()
    return m, [ref_d, len_d]


def stage(c, call):
    """vbz_gpu_match_batch over one call of the catalogue -> uint32 [reads, R, 2]; the guard row behind the hits keeps its canary"""
    query, valid, ref, ref_len = call.arrays()
    n, R = len(query), len(ref)
    m, keep = match_struct(c, call.N, call.quant, ref, ref_len)
    q = torch.from_numpy(query).to(c.device)
    v = i32(valid).to(c.device)
    out = torch.full((n + 1, R, 2), HIT_CANARY, dtype=torch.int32, device=c.device)
    torch.cuda.synchronize()
    rc = c.L.vbz_gpu_match_batch(c.ctx, n, q.data_ptr(), v.data_ptr(), ctypes.byref(m), out.data_ptr())
    c.synchronize()
    assert rc == 0, c.L.vbz_gpu_last_error(c.ctx)
    got = out.cpu().numpy().view(np.uint32)
    assert (got[n] == HIT_CANARY).all(), "hits behind the last read were written"
    assert (q.cpu().numpy().view(np.uint32) == query.view(np.uint32)).all(), "the stage entry wrote its query"
    return got[:n]


def assert_hits(got, want, what):
    bad = np.argwhere((got != want).any(axis=-1))
    assert bad.size == 0, (what, "read, reference", bad[:6].tolist(), "got", [got[tuple(b)].tolist() for b in bad[:6]], "want",
                           [want[tuple(b)].tolist() for b in bad[:6]])


def query_rows(sig, bg, en, N, consts=None, norm=None, stats=0):
    """every read's query row (uint32 bits [n, N]) and, with norm, its (shift, scale); T' per read"""
    rows, ss, Tp = [], [], []
    for i, x in enumerate(sig):
        b, e = G.clamp(len(x), bg[i], en[i])
        Tp.append(e - b)
        if norm is not None:
            row, shift, scale = W.norm_window_rows(x, bg[i], en[i], [0], N, norm, stats, 0.0, "f32")
            ss.append((shift, scale))
        else:
            row = W.window_rows(x, bg[i], en[i], [0], N, consts[i][0], consts[i][1], 0.0, "f32")
        rows.append(row[0])
    return np.stack(rows) if rows else np.zeros((0, N), np.uint32), ss, Tp


class Arenas:
    """canary-filled query, hits and shift_scale of n reads, a guard row behind each"""

    def __init__(self, c, n, N, R):
        self.n, self.N, self.R = n, N, R
        self.query = torch.full((n + 1, N), Q_CANARY, dtype=torch.float32, device=c.device)
        self.out = torch.full((n + 1, R, 2), HIT_CANARY, dtype=torch.int32, device=c.device)
        self.ss = torch.full((n + 1, 2), SS_CANARY, dtype=torch.float32, device=c.device)

    def untouched(self):
        return ((self.query.cpu().numpy() == Q_CANARY).all() and (self.out.cpu().numpy().view(np.uint32) == HIT_CANARY).all()
                and (self.ss.cpu().numpy() == SS_CANARY).all())

    def check(self, want_q, want_ss, Tp, quant, ref, ref_len, failed, what):
        """the query's bits, the hits of that query, shift_scale, the guard rows.  failed: reads whose verdict is an error -- the empty
        verdict in every column, the query row unspecified"""
        n, N = self.n, self.N
        q = self.query.cpu().numpy()
        got_q = q.view(np.uint32)
        ok = [i for i in range(n) if i not in failed]
        bad = np.argwhere(got_q[ok] != want_q[ok])
        assert bad.size == 0, (what, "query: read (among the passing), position", bad[:4].tolist())
        assert (q[n] == Q_CANARY).all(), "the query row behind the last read was written"
        valid = [0 if i in failed else min(Tp[i], N) for i in range(n)]
        want = M.hits(want_q.view(np.float32), valid, quant, ref, ref_len)
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


class MatchRun:
    """one raw vbz_gpu_signal_match_batch call and its check.  ref / ref_len: the reference matrix and its lengths"""

    def __init__(self, fr, ref, ref_len, N, quant=32.0, begin=None, end=None, norm=None, stats=0, signed=True, offset=None, scale=None, src=None):
        c = fr.c
        self.fr, self.ref, self.ref_len, self.N, self.quant, self.norm, self.stats, self.signed = fr, ref, ref_len, N, quant, norm, stats, signed
        n, dev = fr.n, c.device
        self.bg, self.en = full(begin, n), full(end, n)
        self.a = Arenas(c, n, N, len(ref))
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
        self.rc = c.L.vbz_gpu_signal_match_batch(c.ctx, ctypes.byref(b), ctypes.byref(fr.opts), int(fr.sized), ctypes.byref(f),
                                                 ctypes.byref(m) if m is not None else None, self.a.ss.data_ptr() if m is not None else None,
                                                 ctypes.byref(g) if (begin is not None or end is not None) else None, ctypes.byref(mt),
                                                 self.a.query.data_ptr(), self.a.out.data_ptr())
        c.synchronize()
        self.err = c.L.vbz_gpu_last_error(c.ctx)

    def values(self, i):
        x = self.fr.reads[i]
        return x if self.signed else x.view(np.uint16)

    def check(self, expect=None):
        """verdicts (expect[i]: another verdict than T x 4 -- an error: the read's hits are the empty verdict), the query, the hits"""
        assert self.rc == 0, self.err
        fr = self.fr
        res = u32(self.result)
        failed = set()
        for i in range(fr.n):
            want = fr.T[i] * 4 if not (expect and i in expect) else expect[i]
            assert int(res[i]) == want, (i, hex(int(res[i])), hex(want))
            if _lib.is_error(want):
                failed.add(i)
        sig = [self.values(i) for i in range(fr.n)]
        want_q, want_ss, Tp = query_rows(sig, self.bg, self.en, self.N, list(zip(self.o, self.s)), self.norm[0] if self.norm else None, self.stats)
        self.want = self.a.check(want_q, want_ss, Tp, self.quant, self.ref, self.ref_len, failed, ("N", self.N, "T", fr.T[:8]))
        return self


class MatchCall(Call):
    """one raw vbz_gpu_pod5_signal_match_batch call over POD5 reads of several rows"""

    def __init__(self, c, frames, rows, first, ref, ref_len, N, quant=32.0, begin=None, end=None, norm=None, stats=0, table=None, **kw):
        super().__init__(c, frames, [len(x) for x in rows], PR.bounds(first, len(rows)) if table is None else table, "f32", None, norm=norm, **kw)
        self.sig = G.pod5_signals(rows, first)
        self.ref, self.ref_len, self.N, self.quant, self.stats = ref, ref_len, N, quant, stats
        n = len(first)
        self.bg, self.en = full(begin, n), full(end, n)
        self.a = Arenas(c, n, N, len(ref))
        self.mt, self.mkeep = match_struct(c, N, quant, ref, ref_len)
        self.g, self.gkeep = ranges_struct(c, begin, end, stats)
        self.ranged = begin is not None or end is not None

    def call(self, read_result=True):
        if not read_result:
            self.reads.read_result = None
        m = ctypes.byref(self.m) if self.m is not None else None
        rc = self.c.L.vbz_gpu_pod5_signal_match_batch(self.c.ctx, ctypes.byref(self.b), ctypes.byref(self.opts), ctypes.byref(self.f), ctypes.byref(self.reads),
                                                      m, self.a.ss.data_ptr() if self.m is not None else None,
                                                      ctypes.byref(self.g) if self.ranged else None, ctypes.byref(self.mt), self.a.query.data_ptr(),
                                                      self.a.out.data_ptr())
        self.c.synchronize()
        return rc

    def check(self, norm=None, consts=None, failed=()):
        want_q, want_ss, Tp = query_rows(self.sig, self.bg, self.en, self.N, consts, norm, self.stats)
        self.want = self.a.check(want_q, want_ss, Tp, self.quant, self.ref, self.ref_len, set(failed), ("pod5", "N", self.N))
        return self
