"""What vbz_gpu_events_query_batch and vbz_gpu_locate_levels_batch refuse on the host (include/vbz_gpu.h): -2 with nothing launched and the
canary-filled arenas untouched -- NULL structs and tables while the call has reads or pairs, flags and reserved, lengths outside their rule,
misalignment, implausible extents.  The same arguments, unspoilt, run; a call of no reads or no pairs is queued and writes nothing."""
import ctypes

import numpy as np
import pytest
import torch

import eventalign_ref as E
from eventalign_support import LevelTables, QueryArenas, assert_levels, assert_query, dev_u32, events_of, records_of
from typed_support import codec
from vbz_compression_amd import _lib

pytestmark = pytest.mark.gpu


class QuerySetup:
    def __init__(self):
        c = self.c = codec()
        self.call = [t for t in E.query_tables() if t.name == "an error verdict"][0]
        self.reads = len(self.call.first) - 1
        self.ev, self.keep = events_of(c, self.call.first, self.call.event_rows)
        self.rec = records_of(c, self.call.mean, self.call.n)
        self.res = dev_u32(c, self.call.result)
        self.a = QueryArenas(c, self.reads, self.call.N)

    def run(self, reads=None, result="ok", ev="ok", records="ok", q="ok", query="ok", valid="ok", index="ok"):
        c, a = self.c, self.a
        pick = lambda v, p: p if isinstance(v, str) else v   # noqa: E731
        qs = _lib.GpuEventsQuery(self.call.N, self.call.min_n, 0, 0)
        evp = ctypes.byref(self.ev) if isinstance(ev, str) else (ctypes.byref(ev) if ev is not None else None)
        qp = ctypes.byref(qs) if isinstance(q, str) else (ctypes.byref(q) if q is not None else None)
        rc = c.L.vbz_gpu_events_query_batch(c.ctx, self.reads if reads is None else reads, pick(result, self.res.data_ptr()), evp, pick(records, self.rec.data_ptr()),
                                            qp, pick(query, a.query.ptr()), pick(valid, a.valid.ptr()), pick(index, a.index.ptr()))
        return rc, c.L.vbz_gpu_last_error(c.ctx).decode()


def refused(got, text):
    rc, msg = got
    assert rc == -2 and text in msg, (rc, msg, text)


def test_events_query_refusals_launch_nothing():
    s = QuerySetup()
    N = s.call.N
    refused(s.run(ev=None), "events is NULL")
    refused(s.run(q=None), "events query is NULL")
    for name in ("records", "query", "valid"):
        refused(s.run(**{name: None}), "is NULL")
    ev2, keep2 = events_of(s.c, s.call.first, s.call.event_rows)
    ev2.event_first = None
    refused(s.run(ev=ev2), "is NULL")
    for n in (0, 4, 12, 65544, 1 << 31):
        refused(s.run(q=_lib.GpuEventsQuery(n, 0, 0, 0)), "outside the rules")
    refused(s.run(q=_lib.GpuEventsQuery(N, 0, 1, 0)), "outside the rules")
    refused(s.run(q=_lib.GpuEventsQuery(N, 0, 0, 1)), "outside the rules")
    for kw in ({"flags": 1}, {"reserved": 1}):
        refused(s.run(ev=events_of(s.c, s.call.first, s.call.event_rows, **kw)[0]), "events outside the rules")
    refused(s.run(query=s.a.query.ptr() + 4), "not 16-byte aligned")
    refused(s.run(records=s.rec.data_ptr() + 8), "not 16-byte aligned")
    refused(s.run(index=s.a.index.ptr() + 4), "not 16-byte aligned")
    refused(s.run(reads=0xFFFFFFFF, q=_lib.GpuEventsQuery(65536, 0, 0, 0)), "not plausible")          # n_reads * N * 4 beyond 2^46
    refused(s.run(ev=events_of(s.c, s.call.first, (1 << 42) + 1)[0]), "not plausible")                # event_rows * 16 beyond 2^46
    assert s.run(reads=0, records=None, query=None, valid=None, index=None, result=None)[0] == 0     # no reads: queued, NULL tables allowed
    refused(s.run(reads=0, q=_lib.GpuEventsQuery(12, 0, 0, 0)), "outside the rules")                  # bad arguments stay refused
    assert s.c.L.vbz_gpu_events_query_batch(None, 0, None, None, None, None, None, None, None) == -1
    torch.cuda.synchronize()
    assert s.a.untouched()
    # records may be NULL when the events declare no rows
    first0 = np.zeros(s.reads + 1, np.uint64)
    assert s.run(ev=events_of(s.c, first0, 0)[0], records=None)[0] == 0
    s.c.synchronize()
    got = s.a.read()
    assert not got[0].any() and not got[1].any() and not got[2].any()
    # ... and the same arguments, unspoilt, run
    assert s.run()[0] == 0
    s.c.synchronize()
    assert_query(s.a.read(), s.call.expected(), s.call)


class LevelSetup:
    def __init__(self):
        self.c = codec()
        self.call = E.levels_tables()[0]
        self.t = LevelTables(self.c, self.call)

    def run(self, n_pairs=None, n_reads=None, N=None, W=None, ev="ok", **tables):
        c, t = self.c, self.t
        ptr = {"pairs": t.pairs.data_ptr(), "hit": t.hit.data_ptr(), "rows": t.rows.data_ptr(), "index": t.index.data_ptr(), "records": t.records.data_ptr(),
               "moments": t.moments.data_ptr(), "n_levels": t.n_levels.ptr(), "levels": t.levels.ptr()}
        ptr.update(tables)
        evp = ctypes.byref(t.ev) if isinstance(ev, str) else (ctypes.byref(ev) if ev is not None else None)
        rc = c.L.vbz_gpu_locate_levels_batch(c.ctx, t.P if n_pairs is None else n_pairs, t.n_reads if n_reads is None else n_reads, t.N if N is None else N,
                                             t.W if W is None else W, ptr["pairs"], ptr["hit"], ptr["rows"], ptr["index"], evp, ptr["records"], ptr["moments"],
                                             ptr["n_levels"], ptr["levels"])
        return rc, c.L.vbz_gpu_last_error(c.ctx).decode()

    def events(self, start=True, **kw):
        pairs, hit, rows, index, first, event_rows, start_, n, moments, n_reads = self.call.arrays()
        rows_declared = kw.pop("event_rows", event_rows)
        return events_of(self.c, first, rows_declared, start_ if start else None, **kw)


def test_locate_levels_refusals_launch_nothing():
    s = LevelSetup()
    refused(s.run(ev=None), "events is NULL")
    for name in ("pairs", "hit", "rows", "records", "moments", "n_levels", "levels"):
        refused(s.run(**{name: None}), "is NULL")
    ev2, keep2 = s.events()
    ev2.event_first = None
    refused(s.run(ev=ev2), "is NULL")
    ev3, keep3 = s.events(start=False)   # start is REQUIRED here
    refused(s.run(ev=ev3), "is NULL")
    for kw in ({"flags": 1}, {"reserved": 1}):
        ev4, keep4 = s.events(**kw)
        refused(s.run(ev=ev4), "events outside the rules")
    for name in ("pairs", "hit", "rows", "records", "moments", "levels"):
        base = {"pairs": s.t.pairs, "hit": s.t.hit, "rows": s.t.rows, "records": s.t.records, "moments": s.t.moments}
        p = s.t.levels.ptr() if name == "levels" else base[name].data_ptr()
        refused(s.run(**{name: p + 8}), "not 16-byte aligned")
    for n in (0, 4, 12, 65544, 1 << 31):
        refused(s.run(N=n), "outside the rules")
        refused(s.run(W=n), "outside the rules")
    refused(s.run(n_pairs=0xFFFFFFFF, W=65536), "not plausible")      # n_pairs * max_width * 32 beyond 2^46
    refused(s.run(n_pairs=0xFFFFFFFF, N=65536, W=8), "not plausible")  # n_pairs * query_len * 8
    refused(s.run(n_reads=0xFFFFFFFF, N=65536), "not plausible")       # n_reads * query_len * 4
    ev5, keep5 = s.events(event_rows=(1 << 42) + 1)
    refused(s.run(ev=ev5), "not plausible")                            # event_rows * 16
    assert s.run(n_pairs=0, pairs=None, hit=None, rows=None, index=None, records=None, moments=None, n_levels=None, levels=None)[0] == 0
    refused(s.run(n_pairs=0, W=12), "outside the rules")
    assert s.c.L.vbz_gpu_locate_levels_batch(None, 0, 0, 8, 8, None, None, None, None, None, None, None, None, None) == -1
    torch.cuda.synchronize()
    assert s.t.n_levels.untouched() and s.t.levels.untouched()
    # ... and the same arguments, unspoilt, run
    assert s.run()[0] == 0
    s.c.synchronize()
    assert_levels(s.t.read(), s.call.expected(), s.call)
