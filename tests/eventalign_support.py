"""The raw event-space alignment calls for the tests on the MI355X (test_gpu_events_query, test_gpu_locate_levels,
test_gpu_eventalign_refusals): one call of eventalign_ref's catalogues into arenas with canary words in front of and behind each, and its
check against the numpy statement bit for bit.  A plain module: every assert carries its operands."""
import ctypes

import numpy as np
import torch

from match_support import HIT_CANARY
from typed_support import i32
from vbz_compression_amd import _lib

GUARD = 64   # canary words on either side of an arena (a multiple of 4: the arena stays 16-byte aligned)


class Guarded:
    """an int32 arena of `words` words between two guards, every word the canary"""

    def __init__(self, c, words):
        self.words = int(words)
        self.t = torch.full((self.words + 2 * GUARD,), HIT_CANARY, dtype=torch.int32, device=c.device)

    def ptr(self):
        return self.t.data_ptr() + 4 * GUARD

    def read(self, what):
        got = self.t.cpu().numpy().view(np.uint32)
        assert (got[:GUARD] == HIT_CANARY).all() and (got[GUARD + self.words:] == HIT_CANARY).all(), "the words around %s were written" % what
        return got[GUARD:GUARD + self.words]

    def untouched(self):
        return bool((self.t.cpu().numpy().view(np.uint32) == HIT_CANARY).all())


def dev_u32(c, a):
    return i32(np.asarray(a, np.uint64).reshape(-1)).to(c.device)


def dev_u64(c, a):
    return torch.from_numpy(np.asarray(a, np.uint64).reshape(-1).view(np.int64).copy()).to(c.device)


def events_of(c, first, event_rows, start=None, flags=0, reserved=0):
    """(vbz_gpu_events, its tables); start None: the struct's NULL"""
    first_d = dev_u64(c, first)
    start_d = dev_u32(c, start) if start is not None else None
    ev = _lib.GpuEvents()
    ev.event_rows, ev.event_first, ev.flags, ev.reserved = int(event_rows), first_d.data_ptr(), flags, reserved
    ev.start = start_d.data_ptr() if start_d is not None and len(start) else None
    return ev, [first_d, start_d]


def records_of(c, mean, n):
    """the event call's arena of {mean, sd, n, 0}; sd carries a pattern nobody may copy"""
    rec = np.zeros((len(n), 4), np.uint32)
    rec[:, 0], rec[:, 1], rec[:, 2] = mean, 0x3F800000, n
    return dev_u32(c, rec)


class QueryArenas:
    def __init__(self, c, reads, N, use_index=True):
        self.reads, self.N = reads, N
        self.query, self.valid = Guarded(c, reads * N), Guarded(c, reads)
        self.index = Guarded(c, reads * N) if use_index else None

    def read(self):
        ix = self.index.read("index").reshape(self.reads, self.N) if self.index else None
        return self.query.read("query").reshape(self.reads, self.N), self.valid.read("valid"), ix

    def untouched(self):
        return self.query.untouched() and self.valid.untouched() and (self.index is None or self.index.untouched())


def stage_query(c, call):
    """vbz_gpu_events_query_batch over one eventalign_ref.QueryCall -> (query, valid, index or None) as uint32"""
    reads = len(call.first) - 1
    ev, keep = events_of(c, call.first, call.event_rows)
    rec = records_of(c, call.mean, call.n)
    res = dev_u32(c, call.result) if call.result is not None else None
    a = QueryArenas(c, reads, call.N, call.use_index)
    q = _lib.GpuEventsQuery(call.N, call.min_n, 0, 0)
    torch.cuda.synchronize()
    rc = c.L.vbz_gpu_events_query_batch(c.ctx, reads, res.data_ptr() if res is not None else None, ctypes.byref(ev), rec.data_ptr() if len(call.n) else None,
                                        ctypes.byref(q), a.query.ptr(), a.valid.ptr(), a.index.ptr() if a.index else None)
    c.synchronize()
    assert rc == 0, c.L.vbz_gpu_last_error(c.ctx)
    return a.read()


def assert_query(got, want, call):
    for name, g, w in zip(("query", "valid", "index"), got, want):
        if g is None:
            continue
        bad = np.argwhere(g != w)
        assert bad.size == 0, (call.name, name, bad[:6].tolist(), [hex(int(g[tuple(b)])) for b in bad[:6]], [hex(int(w[tuple(b)])) for b in bad[:6]])


class LevelTables:
    """the device tables of one eventalign_ref.LevelsCall"""

    def __init__(self, c, call):
        pairs, hit, rows, index, first, event_rows, start, n, moments, self.n_reads = call.arrays()
        self.P, self.N, self.W = len(pairs), call.N, call.W
        self.pairs, self.hit, self.rows = dev_u32(c, pairs), dev_u32(c, hit), dev_u32(c, rows)
        self.index = dev_u32(c, index) if index is not None else None
        self.ev, self.keep = events_of(c, first, event_rows, start)
        self.records = records_of(c, np.arange(len(n)) * 2654435761 % (1 << 32), n)
        self.moments = dev_u64(c, moments)
        self.rows_total = len(n)
        self.n_levels, self.levels = Guarded(c, self.P), Guarded(c, self.P * self.W * 8)

    def call(self, c, W=None):
        return c.L.vbz_gpu_locate_levels_batch(c.ctx, self.P, self.n_reads, self.N, self.W if W is None else W, self.pairs.data_ptr(), self.hit.data_ptr(),
                                               self.rows.data_ptr(), self.index.data_ptr() if self.index is not None else None, ctypes.byref(self.ev),
                                               self.records.data_ptr() if self.rows_total else None, self.moments.data_ptr() if self.rows_total else None,
                                               self.n_levels.ptr(), self.levels.ptr())

    def read(self):
        return self.n_levels.read("n_levels"), self.levels.read("levels").reshape(self.P, self.W, 8)


def stage_levels(c, call):
    """vbz_gpu_locate_levels_batch over one eventalign_ref.LevelsCall -> (n_levels uint32 [pairs], levels uint32 [pairs, W, 8])"""
    t = LevelTables(c, call)
    torch.cuda.synchronize()
    rc = t.call(c)
    c.synchronize()
    assert rc == 0, c.L.vbz_gpu_last_error(c.ctx)
    return t.read()


def assert_levels(got, want, call):
    (gn, gl), (wn, wl) = got, want
    bad = np.flatnonzero(gn != wn)
    assert bad.size == 0, (call.name, "n_levels of pairs", [(int(p), call.hit[p], int(gn[p]), int(wn[p])) for p in bad[:6]])
    bad = np.argwhere((gl != wl).any(axis=-1))
    assert bad.size == 0, (call.name, "levels: pair, level", bad[:6].tolist(), [call.hit[p] for p, _ in bad[:3]], "got", [gl[tuple(b)].tolist() for b in bad[:4]],
                           "want", [wl[tuple(b)].tolist() for b in bad[:4]])
